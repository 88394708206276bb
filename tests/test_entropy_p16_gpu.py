"""The pictures of p16_fast, the P_L0_16x16 path of the two CABAC-only I/P entropy kernels (k_entropy.hip under MI_ENT_P16): a macroblock of
that type decodes ref_idx_l0, mvd_l0 and coded_block_pattern from the left / upper neighbour entries alone, predicts its vector from the four
neighbour entries and, without residual, writes record and edge entry from registers; with residual it joins the general road at mb_qp_delta.

A RECIPE here is one kind of content in all five GEOMETRIES -- one macroblock (no neighbour at all), one row (nothing above), one column (nothing
to the left, C never there), 2 x 2 and QCIF -- as the five streams of one batch, 4 .. 6 pictures each.  Every recipe is decoded three ways, as in
test_entropy_main_gpu.py: alone (level 0 on k_entropy_m), next to a stream with the 8x8 transform (k_entropy_c) and next to a CAVLC stream
(k_entropy, the road that has no such path), each time against the generator's reconstruction, bit for bit; the side-information planes (K11)
of the first decode are held against the oracle's macroblock trace.  No tolerance anywhere.

Reach: a one-macroblock picture has five P macroblocks in six pictures, so the counts hold per recipe, over its five streams -- at least 20
P_L0_16x16 macroblocks without residual and at least 10 with, counted on the CPU from the oracle's trace (test_recipes_reach_both_exits, which
needs no GPU; the seeds below were chosen so that the generator alone meets it)."""
import numpy as np
import pytest

from conftest import MATRIX
from test_entropy_main_gpu import CABAC, GENERAL, MAIN, _decode, _gen, _route

GEOMETRIES = ((16, 16), (176, 16), (16, 144), (32, 32), (176, 144))
COMMON = dict(profile_idc=77, cabac=1, idr_period=0, skip_permille=150)
RECIPES = {
    # global motion by whole samples / by quarter samples in both directions
    "whole_motion": dict(motion_x4=8, motion_y4=-4, qp=30, seed=701),
    "frac_motion": dict(motion_x4=11, motion_y4=-6, qp=30, seed=702),
    # vectors far from their predictors: mvd beyond the prefix of 9 (Exp-Golomb suffix), context sums below 3, in 3..32 and above 32
    "large_mvd": dict(motion_x4=37, motion_y4=-29, mv_reach=400, mv_margin=64, qp=30, seed=703),
    # three reference pictures: ref_idx_l0 bins, contexts from A and B
    "multiref": dict(num_ref_frames=3, qp=30, seed=704),
    # three slices per picture that start in the middle of a row (intra_stim splits by macroblock count): neighbours of another slice are not there
    "slices3_midrow": dict(slices=3, intra_stim=1, cabac_init_idc=-1, num_ref_frames=3, qp=30, seed=705),
    # intra macroblocks at A, B and C of many P_L0_16x16 macroblocks
    "intra_neighbours": dict(intra_in_p_permille=350, qp=30, seed=706),
    # 8x8 and smaller partitions around: D's mv[3] / ref[1] differ from the entry's first
    "sub8x8_around": dict(sub8x8_permille=600, skip_permille=100, num_ref_frames=2, qp=33, seed=707),
    # low QP: about half of the P_L0_16x16 macroblocks carry residual (the hand-over), QP moving from macroblock to macroblock
    "lowqp_dqp": dict(qp=26, qp_jitter=5, seed=708),
}
MIN_WITHOUT, MIN_WITH = 20, 10


def recipe_kw(name, geo):
    kw = dict(COMMON, width=geo[0], height=geo[1], frames=4 if geo == (176, 144) else 6, **RECIPES[name])
    kw["seed"] += 10 * GEOMETRIES.index(geo)
    if geo != (176, 144):
        kw["qp"] += 6  # (the small pictures are mostly border: a coarser quantiser leaves some of their macroblocks without residual)
    if kw.get("slices", 1) > 1:
        kw["slices"] = min(kw["slices"], (geo[0] // 16) * (geo[1] // 16))
    return kw


_cache = {}


def streams_of(sg, name):
    """[(kw, stream, rec, ranges)] of a recipe, generated once per run and left unchanged"""
    if name not in _cache:
        out = []
        for geo in GEOMETRIES:
            kw = recipe_kw(name, geo)
            stream, rec, _ = sg.encode(**kw)
            rec.setflags(write=False)
            out.append((kw, stream, rec, sg.last_ranges()))
        _cache[name] = out
    return _cache[name]


def trace_of(oracle, stream, kw):
    """the oracle's macroblock trace as [picture, row, column, 8]: raw mb_type (-1 skipped), cbp, QP_Y, mode, t8x8, mv[0] x / y, ref_idx of block 0"""
    frames, info, tr = oracle.decode(stream, crop=False, trace=True)
    wmb, hmb = kw["width"] // 16, kw["height"] // 16
    assert tr.shape[0] == kw["frames"] * wmb * hmb
    return frames, tr.reshape(kw["frames"], hmb, wmb, 8)


def count_p16(oracle, stream, kw, rec):
    """(P_L0_16x16 macroblocks without residual, with residual, of the latter: with a QP other than the macroblock's before it in the slice)"""
    frames, tr = trace_of(oracle, stream, kw)
    assert np.array_equal(frames, rec), "oracle != generator: the trace is no yardstick"
    p16 = (tr[..., 0] == 0) & (tr[..., 7] >= 0)  # raw mb_type 0 with a reference: not the I_NxN of an I slice
    with_res = p16 & (tr[..., 1] != 0)
    flat_qp, flat_res = tr[..., 2].reshape(kw["frames"], -1), with_res.reshape(kw["frames"], -1)
    dqp = int((flat_res[:, 1:] & (flat_qp[:, 1:] != flat_qp[:, :-1])).sum())
    return int((p16 & (tr[..., 1] == 0)).sum()), int(with_res.sum()), dqp


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipes_reach_both_exits(name, sg, oracle_mod):
    """On the CPU: every recipe has P_L0_16x16 macroblocks without residual (the register write-out) and with (the hand-over) in numbers, and what
    its name promises."""
    without = with_res = dqp = 0
    mvd = [0, 0]
    for kw, stream, rec, ranges in streams_of(sg, name):
        a, b, c = count_p16(oracle_mod, stream, kw, rec)
        print("%s %dx%d: %d without residual, %d with (%d of them after a QP change); largest |mvd| %d, %d" %
              (name, kw["width"], kw["height"], a, b, c, ranges["mvd_max_x"], ranges["mvd_max_y"]))
        without, with_res, dqp = without + a, with_res + b, dqp + c
        mvd = [max(mvd[0], ranges["mvd_max_x"]), max(mvd[1], ranges["mvd_max_y"])]
    assert without >= MIN_WITHOUT and with_res >= MIN_WITH, (name, without, with_res)
    if name == "large_mvd":
        assert min(mvd) > 32, mvd  # one neighbour alone takes the context sum past 32; the suffix starts at 9
    if name == "lowqp_dqp":
        assert dqp >= 1 and with_res * 3 >= without, (dqp, without, with_res)


def _check_side(H, oracle, dec, items):
    """type, nz, mvx0, mvy0, ref0 of every macroblock's first block (nz: of all sixteen) against the oracle's trace"""
    views = dec.side_info(planes=("type", "nz", "mvx0", "mvy0", "ref0"))
    at = 0
    for kw, stream, _, _ in items:
        _, tr = trace_of(oracle, stream, kw)
        for f in range(kw["frames"]):
            v = views[at].cpu().numpy()
            at += 1
            typ, nz, mvx, mvy, ref = (v[k] for k in range(5))
            t = tr[f]
            p16, skip = (t[..., 0] == 0) & (t[..., 7] >= 0), t[..., 0] == -1
            assert ((typ[::4, ::4] == H.MB_P16x16) == p16).all() and ((typ[::4, ::4] == H.MB_PSKIP) == skip).all(), (kw, f)
            inter = t[..., 7] >= 0
            assert np.array_equal(mvx[::4, ::4][inter], t[..., 5][inter]) and np.array_equal(mvy[::4, ::4][inter], t[..., 6][inter]), (kw, f)
            assert np.array_equal(ref[::4, ::4][inter], t[..., 7][inter]), (kw, f)
            for arr in (mvx, mvy, ref):  # one partition: the sixteen blocks of a P_L0_16x16 macroblock are alike
                blocks = arr.reshape(arr.shape[0] // 4, 4, arr.shape[1] // 4, 4).transpose(0, 2, 1, 3)[p16]  # [macroblock, 4, 4]
                assert (blocks == blocks[:, :1, :1]).all(), (kw, f)
            none = np.repeat(np.repeat(t[..., 1] == 0, 4, axis=0), 4, axis=1)
            assert (nz[none] == 0).all(), (kw, f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RECIPES))
def test_gpu_p16_three_routes_give_the_generators_pictures(name, H, sg, oracle_mod):
    items = streams_of(sg, name)
    without = with_res = 0
    for kw, stream, rec, _ in items:
        a, b, _ = count_p16(oracle_mod, stream, kw, rec)
        without, with_res = without + a, with_res + b
    assert without >= MIN_WITHOUT and with_res >= MIN_WITH, (name, without, with_res)
    pairs = [(kw, stream) for kw, stream, _, _ in items]
    kws = [kw for kw, _ in pairs]
    t8_kw, cav_kw = MATRIX["high8x8_cabac"], MATRIX["cavlc_I"]
    assert _route(H, kws) == MAIN and _route(H, kws + [t8_kw]) == CABAC and _route(H, kws + [cav_kw]) == GENERAL
    t8, t8_rec = _gen(sg, "high8x8_cabac")
    cav, cav_rec = _gen(sg, "cavlc_I")
    # alone: k_entropy_m; the decoder is kept for the side-information planes
    W, Hc = max(kw["width"] for kw in kws), max(kw["height"] for kw in kws)
    dec = H.Decoder(max_streams=len(pairs), max_width=W, max_height=Hc, max_frames_per_batch=max(kw["frames"] for kw in kws),
                    max_slices_per_frame=max(kw.get("slices", 1) for kw in kws), max_bitstream_bytes=sum(len(s) for _, s in pairs) * 2 + (1 << 20))
    try:
        dec.decode([s for _, s in pairs])
        for i, (kw, _, rec, _) in enumerate(items):
            out = dec.read_frames(i, crop=True, size=kw["width"] * kw["height"] * 3 // 2)
            assert out.shape == rec.shape and np.array_equal(out, rec), "k_entropy_m != generator reconstruction: %dx%d" % (kw["width"], kw["height"])
        _check_side(H, oracle_mod, dec, items)
    finally:
        dec.close()
    with8 = _decode(H, pairs + [(t8_kw, t8)])      # one stream with the 8x8 transform in the batch: k_entropy_c
    mixed = _decode(H, pairs + [(cav_kw, cav)])    # one CAVLC slice in the launch: k_entropy
    for i, (kw, _, rec, _) in enumerate(items):
        assert np.array_equal(with8[i], rec), "k_entropy_c != generator reconstruction: %dx%d" % (kw["width"], kw["height"])
        assert np.array_equal(mixed[i], rec), "k_entropy != generator reconstruction: %dx%d" % (kw["width"], kw["height"])
    assert np.array_equal(with8[-1], t8_rec) and np.array_equal(mixed[-1], cav_rec)


@pytest.mark.gpu
def test_gpu_p16_damaged_slice_ends_in_order(H, sg):
    """One byte of the second picture's slice data flipped in a stream whose P macroblocks are mostly P_L0_16x16, no concealment: the call returns,
    the stream's status is 0 (the damage decoded as something) or H264MI_ECORRUPT (-8), the intact stream beside it is exact."""
    kw, stream, rec, _ = streams_of(sg, "lowqp_dqp")[-1]
    good_kw, good, good_rec, _ = streams_of(sg, "frac_motion")[-1]
    assert _route(H, [kw, good_kw]) == MAIN
    nals = H.read_nal_units(stream)
    slices = [i for i, n in enumerate(nals) if n.Type in (1, 5)]
    second = slices[1]
    begin = nals[second].Offset
    end = nals[second + 1].Offset - 4 if second + 1 < len(nals) else len(stream)
    assert end - begin > 64
    b = bytearray(stream)
    b[begin + (end - begin) // 2] ^= 0xFF
    dec = H.Decoder(max_streams=2, max_width=176, max_height=144, max_frames_per_batch=kw["frames"], max_bitstream_bytes=1 << 20)
    try:
        dec.set_isolation(True)
        dec.decode([bytes(b), good])
        status = dec.stream_status(0)
        print("status of the damaged stream: %d" % status)
        assert status in (0, -8)
        assert dec.stream_status(1) == 0
        assert np.array_equal(dec.read_frames(1, crop=True, size=good_kw["width"] * good_kw["height"] * 3 // 2), good_rec)
        assert np.array_equal(dec.read_frames(0, crop=False)[0], rec[0]), "the intact first picture of the damaged stream"
    finally:
        dec.close()
