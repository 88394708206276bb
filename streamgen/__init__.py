"""ctypes wrapper of the synthetic H.264 stream generator (streamgen/).

Input synthesis only: produces Annex-B streams plus the generator's own closed-loop
reconstruction.  Not part of the decode product and not the oracle."""
import ctypes
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "_build", "libstreamgen.so")


class Params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "width", "height", "frames", "profile_idc", "cabac", "qp", "qp_jitter", "idr_period", "slices",
        "transform8x8", "num_ref_frames", "deblock_idc", "alpha_off_div2", "beta_off_div2", "cabac_init_idc",
        "constrained_intra", "chroma_qp_offset", "pcm_permille", "intra_in_p_permille", "skip_permille",
        "sub8x8_permille", "weighted_pred", "scaling_matrix", "noise")] + [("seed", ctypes.c_uint32),
        ("long_start_code", ctypes.c_int), ("poc_type", ctypes.c_int), ("rplm", ctypes.c_int), ("mmco", ctypes.c_int),
        ("idr_long_term", ctypes.c_int), ("nonref_period", ctypes.c_int), ("slice_qp_delta", ctypes.c_int), ("bframes", ctypes.c_int),
        ("direct_temporal", ctypes.c_int), ("weighted_bipred", ctypes.c_int), ("bskip_permille", ctypes.c_int),
        ("motion_x4", ctypes.c_int), ("motion_y4", ctypes.c_int), ("interlace_sps", ctypes.c_int), ("fn_gap_period", ctypes.c_int), ("fn_gap_declared", ctypes.c_int),
        ("b_pyramid", ctypes.c_int), ("slice_groups", ctypes.c_int), ("fmo_type", ctypes.c_int), ("aso", ctypes.c_int), ("field_pics", ctypes.c_int), ("poc_bottom_delta", ctypes.c_int), ("mono", ctypes.c_int),
        ("wp_range", ctypes.c_int), ("poc_step", ctypes.c_int), ("mv_reach", ctypes.c_int), ("mv_margin", ctypes.c_int), ("contrast", ctypes.c_int),
        ("dbf_per_slice", ctypes.c_int), ("trace_deblock", ctypes.c_int), ("syntax_stim", ctypes.c_int),
        ("intra_stim", ctypes.c_int), ("trace_intra", ctypes.c_int),
        ("direct_4x4", ctypes.c_int), ("trace_motion", ctypes.c_int), ("motion_stim", ctypes.c_int), ("open_gop_period", ctypes.c_int),
        ("trace_residual", ctypes.c_int), ("residual_stim", ctypes.c_int)]


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in os.listdir(_HERE) if f.endswith((".c", ".h"))]
    if force or not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
        subprocess.check_call(["make", "-s", "-C", _HERE])
    return _LIB


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(_LIB)
        _lib.sg_encode.restype = ctypes.c_size_t
        _lib.sg_encode.argtypes = [ctypes.POINTER(Params), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                   ctypes.c_size_t, ctypes.c_void_p]
        _lib.sg_default_params.argtypes = [ctypes.POINTER(Params)]
        _lib.sg_last_error.restype = ctypes.c_char_p
        _lib.sg_source_frame.argtypes = [ctypes.POINTER(Params), ctypes.c_int, ctypes.c_void_p]
        _lib.sg_last_pocs.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _lib.sg_last_features.restype = ctypes.c_uint32
        _lib.sg_last_entries.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _lib.sg_last_ranges.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _lib.sg_last_syntax.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _lib.sg_cavlc_level_bits.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        _lib.sg_last_deblock_trace.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        _lib.sg_last_intra_trace.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        _lib.sg_last_motion.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _lib.sg_last_residual_trace.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        _lib.sg_last_motion_trace.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    return _lib


def default_params(**kw):
    p = Params()
    lib().sg_default_params(ctypes.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def encode(want_recon=True, **kw):
    """Returns (stream bytes, recon uint8[frames, coded_h*coded_w*3/2] or None, frame_sizes)."""
    p = default_params(**kw)
    W, H = (p.width + 15) & ~15, (p.height + 15) & ~15
    fsz = W * H * 3 // 2
    cap = max(1 << 20, p.frames * fsz * 2)
    stream = np.zeros(cap, dtype=np.uint8)
    recon = np.zeros((p.frames, fsz), dtype=np.uint8) if want_recon else None
    sizes = np.zeros(p.frames, dtype=np.uint32)
    n = lib().sg_encode(ctypes.byref(p), stream.ctypes.data, cap, recon.ctypes.data if want_recon else None,
                        recon.nbytes if want_recon else 0, sizes.ctypes.data)
    if n == 0:
        raise RuntimeError("streamgen failed: %s" % lib().sg_last_error().decode())
    return stream[:n].tobytes(), recon, sizes


def last_pocs():
    """PicOrderCnt the generator intended for every picture of the last encode() call."""
    n = lib().sg_last_pocs(None, 0)
    out = np.zeros(n, dtype=np.int32)
    lib().sg_last_pocs(out.ctypes.data, n)
    return out


def last_features():
    """Bit set of the picture-management syntax the last encode() call emitted (see sg.h)."""
    return int(lib().sg_last_features())


FEATURE_OPEN_GOP = 1 << 16


def last_entries():
    """The entry points of the last encode(open_gop_period=N, ...): per non-IDR I picture with a recovery point (frame of the reconstruction, i.e. its
    place in coding order; leading pictures that follow it, a field counting as one)."""
    n = lib().sg_last_entries(None, 0)
    out = np.zeros(2 * n, dtype=np.int32)
    lib().sg_last_entries(out.ctypes.data, 2 * n)
    return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)]


RANGE_NAMES = (
    "mvd_max_x", "mvd_max_y", "outside_left", "outside_right", "outside_top", "outside_bottom",
    "half1_clip0", "half1_clip255", "halfj_clip0", "halfj_clip255",
    "w1_clip0", "w1_clip255", "w2_clip0", "w2_clip255", "denom_mask",
    "w_min", "w_max", "o_min", "o_max", "neg_weight", "odd_neg_offsets",
    "tbtd_clipped", "dsf_clipped", "implicit_fallback", "implicit_pairs", "implicit_w1_min", "implicit_w1_max", "scaling_forms", "guard_zeroed", "ref_twice") + tuple(
    # deblocking (the SG_R_DB_* counters)
    "db_%s_%s_bs%d" % (f, pl, b) for pl in ("luma", "chroma") for f in ("filt", "rej") for b in (1, 2, 3, 4)) + (
    "db_rej_alpha", "db_rej_beta_p", "db_rej_beta_q", "db_ap0_aq0", "db_ap0_aq1", "db_ap1_aq0", "db_ap1_aq1",
    "db_delta_lo", "db_delta_hi", "db_delta_in", "db_p1_lo", "db_p1_hi", "db_q1_lo", "db_q1_hi",
    "db_p0_at0", "db_p0_at255", "db_q0_at0", "db_q0_at255", "db_tc0_zero", "db_tc0_zero_ap", "db_bs4_small", "db_bs4_not_small",
    "db_bs4_strong_p0_q0", "db_bs4_strong_p0_q1", "db_bs4_strong_p1_q0", "db_bs4_strong_p1_q1",
    "db_index_a_min", "db_index_a_max", "db_index_b_min", "db_index_b_max", "db_index_a_clip0", "db_index_a_clip51",
    "db_qp_odd", "db_pcm_edge", "db_cbcr_alpha", "db_pair_differs", "db_cbcr_pair_differs", "db_seg_none", "db_field_bs3",
    "db_b_bs1_crossed", "db_b_bs1_straight", "db_b_bs0_crossed", "db_slice_offsets", "db_idc1_modified", "db_idc2_skipped") + tuple(
    # intra prediction (the SG_R_IP_* counters): availability masks per (kind, mode), top-right use per block index, clips, foreign samples
    "ip_av%s_m%d" % (k, m) for k, n in (("4", 9), ("8", 9), ("16", 4), ("c", 4)) for m in range(n)) + tuple(
    "ip_tr%d_b%d" % (k, b) for k, n in ((4, 16), (8, 4)) for b in range(n)) + (
    "ip_plane16_lo", "ip_plane16_hi", "ip_planec_lo", "ip_planec_hi", "ip_rec_luma_at0", "ip_rec_luma_at255", "ip_rec_chroma_at0", "ip_rec_chroma_at255",
    "ip_from_inter", "ip_from_pcm", "ip_f8_top_no_tl", "ip_f8_left_no_tl")


def last_ranges():
    """What the last encode() call really reached (the SG_R_* counters of sg.h), as a dict."""
    n = lib().sg_last_ranges(None, 0)
    assert n == len(RANGE_NAMES), (n, len(RANGE_NAMES))
    out = np.zeros(n, dtype=np.int32)
    lib().sg_last_ranges(out.ctypes.data, n)
    return {k: int(v) for k, v in zip(RANGE_NAMES, out)}


# the SG_S_* words of sg.h: (name, number of words).  Bitmaps of more than 32 bits and tables with several rows are lists of words.
SYNTAX_WORDS = (
    ("token", 15), ("nc_one", 1), ("nc_none", 1), ("tz16", 15), ("tz15", 15), ("tzc", 3), ("run", 7),
    ("prefix_max", 1), ("p14_sl", 1), ("p15_sl", 1), ("p16_sl", 1), ("level_max", 1), ("start_sl1", 1), ("cavlc_8x8_full", 1),
    ("egk_max", 1), ("level_max_cabac", 1), ("cat_blocks", 6), ("last_at_end", 6), ("all_nonzero", 6), ("inc0_sat", 1), ("gt1_sat", 1),
    ("cbf_inc", 5), ("cbf_unavail_intra", 1), ("cbf_unavail_inter", 1),
    ("dqp_min", 1), ("dqp_max", 1), ("dqp_wrap_up", 1), ("dqp_wrap_down", 1), ("qpy_min", 1), ("qpy_max", 1),
    ("dqp_after_skip", 1), ("dqp_after_pcm", 1), ("dqp_after_nodelta", 1), ("qpc_clip0", 1), ("qpc_clip51", 1),
    ("cbp_intra", 2), ("cbp_inter", 2), ("mbtype_i", 1), ("rem4", 1), ("rem8", 1),
    ("skip_run_max", 1), ("end_in_skip", 1), ("end_in_pcm", 1), ("mb_bits_max", 1), ("thinned", 1))
_SIGNED = ("dqp_min", "dqp_max", "qpy_min", "qpy_max")


def last_syntax():
    """What the entropy writers of the last encode() call wrote (the SG_S_* words of sg.h), as a dict: a number per counter, a list of numbers per table;
    bitmaps are unsigned (`token`: five tables of three words, bit 4 * TotalCoeff + TrailingOnes; `cbp_*`: two words)."""
    n = lib().sg_last_syntax(None, 0)
    assert n == sum(k for _, k in SYNTAX_WORDS), (n, sum(k for _, k in SYNTAX_WORDS))
    raw = np.zeros(n, dtype=np.int32)
    lib().sg_last_syntax(raw.ctypes.data, n)
    out, at = {}, 0
    for name, k in SYNTAX_WORDS:
        words = [int(v) if name in _SIGNED else int(v) & 0xFFFFFFFF for v in raw[at:at + k]]
        out[name] = words[0] if k == 1 else words
        at += k
    out["token"] = [sum(w << (32 * i) for i, w in enumerate(out["token"][3 * t:3 * t + 3])) for t in range(5)]
    for k in ("cbp_intra", "cbp_inter"):
        out[k] = out[k][0] | out[k][1] << 32
    return out


def cavlc_level_bits(level, suffix_len, minus2, escape16=1):
    """The bits of one CAVLC coefficient level as the generator writes it, as a string of '0' / '1' (None: the level cannot be written)."""
    bits = ctypes.c_uint64(0)
    n = lib().sg_cavlc_level_bits(level, suffix_len, minus2, escape16, ctypes.byref(bits))
    return None if n < 0 else format(bits.value, "0%db" % n)


# sg_dbmb (sg_int.h), one per macroblock: what 8.7 needs to know about it
DBMB = np.dtype(dict(names=["intra", "t8x8", "qp", "qpc", "dbf_idc", "alpha_off", "beta_off", "slice_id", "nzmask", "mv", "refid", "mv1", "refid1", "pcm"],
                     formats=["u1", "u1", "u1", ("u1", 2), "u1", "i1", "i1", "u2", "u2", ("i2", (16, 2)), ("i4", 4), ("i2", (16, 2)), ("i4", 4), "u1"],
                     offsets=[0, 1, 2, 3, 5, 6, 7, 8, 10, 12, 76, 92, 156, 172], itemsize=176))


def last_deblock_trace():
    """For every picture of the last encode(trace_deblock=1, ...) of this thread, in coding order, a dict: `planes` = (Y, Cb, Cr) before sg_deblock,
    `after` = the same after it, `mbs` = the sg_dbmb table as a structured array [rows, columns] (intra, t8x8, qp, qpc, dbf_idc, alpha_off / beta_off
    = filterOffsetA / B, slice_id, nzmask, refid / refid1 and mv / mv1 per 8x8 / 4x4 block, pcm), `field` = 0 frame / 1 top / 2 bottom field, `mono`,
    `frame` = the frame of the reconstruction the picture belongs to."""
    n = lib().sg_last_deblock_trace(-1, None, None, None, 0, None, 0)
    out = []
    for i in range(n):
        info = np.zeros(8, dtype=np.int32)
        lib().sg_last_deblock_trace(i, info.ctypes.data, None, None, 0, None, 0)
        w, h, wmb, hmb, field, mono, frame, size = (int(v) for v in info)
        assert size == DBMB.itemsize, (size, DBMB.itemsize)
        before, after = np.zeros(w * h * 3 // 2, dtype=np.uint8), np.zeros(w * h * 3 // 2, dtype=np.uint8)
        mbs = np.zeros((hmb, wmb), dtype=DBMB)
        lib().sg_last_deblock_trace(i, None, before.ctypes.data, after.ctypes.data, before.nbytes, mbs.ctypes.data, mbs.nbytes)

        def planes(a):
            return a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), a[w * h * 5 // 4:].reshape(h // 2, w // 2)
        out.append(dict(planes=planes(before), after=planes(after), mbs=mbs, field=field, mono=mono, frame=frame))
    return out


# sg_ipmb (sg.h), one per macroblock: what 8.3 needs to know about it
IPMB = np.dtype(dict(names=["kind", "i16mode", "chroma_mode", "ipm", "slice_id"], formats=["u1", "u1", "u1", ("i1", 16), "u2"], offsets=[0, 1, 2, 4, 20], itemsize=24))
KIND_INTER, KIND_I4, KIND_I8, KIND_I16, KIND_PCM = range(5)


def last_intra_trace():
    """For every picture of the last encode(trace_intra=1, ...) of this thread, in coding order, what last_deblock_trace() gives (`planes` before
    sg_deblock, `after`, `mbs`, `field`, `mono`, `frame`) and: `pred` / `res` = (Y, Cb, Cr) of the prediction (uint8) and residual (int16) sample of every
    intra-predicted sample, 0 elsewhere; `ipmbs` = the sg_ipmb table [rows, columns] (kind: 0 inter, 1 Intra4x4, 2 Intra8x8, 3 Intra16x16, 4 I_PCM; ipm per
    4x4 block at 4 * row + column; i16mode; chroma_mode; slice_id); `constrained_intra`."""
    out = last_deblock_trace()
    for i, t in enumerate(out):
        info = np.zeros(9, dtype=np.int32)
        lib().sg_last_intra_trace(i, info.ctypes.data, None, None, 0, None, 0)
        w, h, wmb, hmb, size = int(info[0]), int(info[1]), int(info[2]), int(info[3]), int(info[7])
        if size == 0:  # a picture kept for trace_deblock alone
            continue
        assert size == IPMB.itemsize, (size, IPMB.itemsize)
        n = w * h * 3 // 2
        pred, res, mbs = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int16), np.zeros((hmb, wmb), dtype=IPMB)
        lib().sg_last_intra_trace(i, None, pred.ctypes.data, res.ctypes.data, n, mbs.ctypes.data, mbs.nbytes)

        def planes(a):
            return a[:w * h].reshape(h, w), a[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), a[w * h * 5 // 4:].reshape(h // 2, w // 2)
        t.update(pred=planes(pred), res=planes(res), ipmbs=mbs, constrained_intra=int(info[8]))
    return out


# sg_rsmb (sg.h), one per macroblock: what 8.5 starts from
RSMB = np.dtype(dict(names=["kind", "t8x8", "cbp", "qp", "slice", "slice_qp", "luma", "dc16", "cdc", "cac", "pcm"],
                     formats=["u1", "u1", "u1", "u1", "u2", "u1", ("i4", (16, 16)), ("i4", 16), ("i4", (2, 4)), ("i4", (2, 4, 15)), ("u1", 384)],
                     offsets=[0, 1, 2, 3, 4, 6, 8, 1032, 1096, 1128, 1608], itemsize=1992))
RS_SKIPPED, RS_INTER, RS_I4, RS_I8, RS_I16, RS_PCM = range(6)


def last_residual_trace():
    """For every picture of the last encode(trace_residual=1, ...) of this thread, in coding order, what last_deblock_trace() gives (`planes` before
    sg_deblock, `after`, `mbs`, `field`, `mono`, `frame`) and: `pred` = (Y, Cb, Cr) of the prediction sample of every sample (inter: after weighting; I_PCM:
    0); `rsmbs` = the sg_rsmb table [rows, columns] (kind RS_*, t8x8, cbp = luma | chroma << 4, qp = QP_Y in force, slice, slice_qp, and the levels as written, in
    scan order: luma [16 blocks in coding order][16] -- Intra16x16: positions 1..15; 8x8 transform: the same numbers as [4][64] --, dc16, cdc [plane][4],
    cac [plane][block][15]; pcm = the 384 samples of an I_PCM macroblock); `chroma_qp_index_offset`, `second_chroma_qp_index_offset`; `lists4` [6][16] and
    `lists8` [2][64] = the scaling lists in force, in the order of their syntax elements."""
    out = last_deblock_trace()
    for i, t in enumerate(out):
        info = np.zeros(10, dtype=np.int32)
        lib().sg_last_residual_trace(i, info.ctypes.data, None, 0, None, 0, None)
        w, h, wmb, hmb, size = int(info[0]), int(info[1]), int(info[2]), int(info[3]), int(info[7])
        if size == 0:  # a picture kept for another trace alone
            continue
        assert size == RSMB.itemsize, (size, RSMB.itemsize)
        n = w * h * 3 // 2
        pred, mbs, lists = np.zeros(n, dtype=np.uint8), np.zeros((hmb, wmb), dtype=RSMB), np.zeros(224, dtype=np.uint8)
        lib().sg_last_residual_trace(i, None, pred.ctypes.data, n, mbs.ctypes.data, mbs.nbytes, lists.ctypes.data)
        t.update(pred=(pred[:w * h].reshape(h, w), pred[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), pred[w * h * 5 // 4:].reshape(h // 2, w // 2)),
                 rsmbs=mbs, chroma_qp_index_offset=int(info[8]), second_chroma_qp_index_offset=int(info[9]),
                 lists4=lists[:96].reshape(6, 16).copy(), lists8=lists[96:].reshape(2, 64).copy())
    return out


# sg_mvmb / sg_mvslice (sg.h): what a derivation of 8.4.1 starts from, and what it must arrive at
MVMB = np.dtype(dict(names=["kind", "raw", "sub", "direct8", "slice", "ref_idx", "mvd", "mv", "ref"],
                     formats=["u1", "i1", ("u1", 4), "u1", "u2", ("i1", (2, 4)), ("i2", (2, 16, 2)), ("i2", (2, 16, 2)), ("i1", (2, 4))],
                     offsets=[0, 1, 2, 6, 8, 10, 18, 146, 274], itemsize=282))
MVSLICE = np.dtype([("type", "i4"), ("direct_spatial", "i4"), ("cur_poc", "i4"), ("first_mb", "i4"), ("count", "i4"), ("nref", "i4", 2),
                    ("pic", "i4", (2, 4)), ("poc", "i4", (2, 4)), ("long_term", "i4", (2, 4)), ("col_index", "i4")])
MV_INTRA, MV_16x16, MV_16x8, MV_8x16, MV_8x8, MV_PSKIP, MV_BDIRECT, MV_BSKIP = range(8)


def last_motion_trace():
    """For every picture of the last encode(trace_motion=1, ...) of this thread, in coding order, a dict: `mbs` = the sg_mvmb table [rows, columns]
    (kind MV_*, raw mb_type, sub_mb_type, direct8, slice, ref_idx and signed mvd as written, and the final mv / ref per list: the thing to be checked),
    `slices` = the sg_mvslice table in sending order (type 0 P / 1 B / 2 I, direct_spatial, cur_poc, first_mb, count, nref and the entries of both
    lists as picture identity `pic`, `poc` and `long_term`, col_index = the index in this list of the picture that is RefPicList1[0]), `field`, `frame`
    = the frame of the reconstruction the picture belongs to, `pic` = the picture's identity."""
    n = lib().sg_last_motion_trace(-1, None, None, 0, None, 0)
    out = []
    for i in range(n):
        info = np.zeros(8, dtype=np.int32)
        lib().sg_last_motion_trace(i, info.ctypes.data, None, 0, None, 0)
        wmb, hmb, field, frame, pic, nsl, msize, ssize = (int(v) for v in info)
        assert (msize, ssize) == (MVMB.itemsize, MVSLICE.itemsize), (msize, ssize, MVMB.itemsize, MVSLICE.itemsize)
        mbs, slices = np.zeros((hmb, wmb), dtype=MVMB), np.zeros(nsl, dtype=MVSLICE)
        lib().sg_last_motion_trace(i, None, mbs.ctypes.data, mbs.nbytes, slices.ctypes.data, slices.nbytes)
        out.append(dict(mbs=mbs, slices=slices, field=field, frame=frame, pic=pic))
    return out


_M_SHAPES = ("med", "16x8u", "16x8l", "8x16l", "8x16r")
_M_RULES = ("dir", "onlyA", "oneA", "oneB", "oneC", "med0", "med2", "med3")
_M_SLOTS = (("P", 0), ("B", 0), ("B", 1))
# the SG_M_* words of sg.h in order: the derivation counters as (cell, ...) names, the syntax words by name
MOTION_NAMES = tuple(("pred", st, lst, shape, rule) for st, lst in _M_SLOTS for shape in _M_SHAPES for rule in _M_RULES) + tuple(
    ("csrc", st, lst, c) for st, lst in _M_SLOTS for c in ("C", "D", "none")) + tuple(
    ("pskip", w) for w in ("A_missing", "B_missing", "A_still", "B_still", "predicted_nonzero", "predicted_zero")) + tuple(
    ("sd_ref", lst, src) for lst in (0, 1) for src in ("A", "B", "C", "none")) + (("sd_bothneg",),) + tuple(
    ("sd_out", lst, o) for lst in (0, 1) for o in ("neg", "zeroed", "kept0", "keptpos_flag")) + (
    ("col", "intra"), ("col", "l0"), ("col", "l1only"), ("td_ref", "zero"), ("td_ref", "pos"), ("td", "long"), ("td", "neg_remainder"),
    "mbtype_p", "mbtype_b", "subtype_p", "subtype_b", "ref_inc", "ref_ge3", "ref_direct_nb", "ref_te1", "ref_ue") + tuple(
    "mvd_band_%s_%d" % (c, b) for c in "xy" for b in range(3)) + ("mvd_suffix", "skip_inc_p", "skip_inc_b", "btype_inc") + tuple(
    ("geo", pos, w) for pos in range(41) for w in ("in_done", "in_later", "B", "C", "outside")) + tuple(("geo_d", pos) for pos in range(41)) + tuple(
    ("nolist", w) for w in ("in_done", "A", "B", "C", "D")) + (("direct_nb", "spatial"), ("direct_nb", "temporal"), ("sd_col", "short"), ("sd_col", "long"),
    ("sd_refcol", "zero"), ("sd_refcol", "pos")) + tuple(("sd_mvcol", c, v) for c in (0, 1) for v in (-2, -1, 0, 1, 2)) + (
    ("col", "corner_differs"), ("col", "four_unlike"), ("td", "mb16"), ("td", "quadrant"))


def last_motion():
    """What the last encode() call did about motion (the SG_M_* words of sg.h), as a dict: the derivation counters under the cell names of
    tests/motionutil.py (tuples), the syntax words under strings (bit masks: mbtype_*, subtype_*, ref_inc, skip_inc_*, btype_inc)."""
    n = lib().sg_last_motion(None, 0)
    assert n == len(MOTION_NAMES), (n, len(MOTION_NAMES))
    out = np.zeros(n, dtype=np.int32)
    lib().sg_last_motion(out.ctypes.data, n)
    return {k: int(v) for k, v in zip(MOTION_NAMES, out)}


SCALING_FORMS = dict(absent_first=1, absent_next=2, use_default=4, cut_short=8, wrap=16, entry_1=32, entry_255=64, full=128,
                     sps_matrix=256, pps_rule_a=512, pps_rule_b=1024, pps_six_lists=2048)

# Named recipes.  Sizes may be overridden for small test cases.
RECIPES = {
    "C1": dict(width=176, height=144, profile_idc=66, cabac=0, frames=30, idr_period=1, qp=28, seed=1),
    "C2": dict(width=1280, height=720, profile_idc=66, cabac=0, frames=60, idr_period=1, qp=28, seed=2),
    "C3": dict(width=1920, height=1080, profile_idc=77, cabac=1, frames=300, idr_period=30, qp=28, seed=3),
    "C4": dict(width=3840, height=2160, profile_idc=100, cabac=1, transform8x8=1, slices=8, frames=120,
               idr_period=30, qp=30, seed=4),
}


def recipe(name, **over):
    kw = dict(RECIPES[name])
    kw.update(over)
    return kw
