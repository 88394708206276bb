"""Inter prediction, the vector syntax and the scaling lists at the ends of their value ranges (recipes: tests/rangeutil.py): explicit weights
over the whole coded range with every denominator, one picture under two weights, PicOrderCnt distances past the clips of 8.4.1.2.3, vectors
out to the limits of Table A-1 with whole prediction windows outside the picture, 0 / 255 content under the 6-tap and the edge filters, coded
scaling lists in the SPS and in changing PPSs.  Generator, oracle and product are three separately written implementations; all three must
agree bit for bit, and the generator's own counters must show that each recipe really goes where it claims to."""
import hashlib
import json
import os

import numpy as np
import pytest

import rangeutil
from rangeutil import RECIPES, decoder_cfg, pictures_of

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "value_range_md5.json")
_cache = {}


def _case(sg, oracle_mod, name):
    """(stream, generator reconstruction, generator PicOrderCnt, counters, oracle frames, oracle PicOrderCnt) of a recipe: made once, not modified"""
    if name not in _cache:
        stream, rec, sizes = sg.encode(**RECIPES[name])
        pocs, ranges = [int(x) for x in sg.last_pocs()], sg.last_ranges()
        ref, _ = oracle_mod.decode(stream, crop=False)
        for a in (rec, ref):
            a.setflags(write=False)
        _cache[name] = (stream, rec, pocs, ranges, ref, [int(x) for x in oracle_mod.last_pocs], sizes)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_oracle_equals_generator(name, sg, oracle_mod):
    stream, rec, pocs, _, ref, ref_pocs, _ = _case(sg, oracle_mod, name)
    assert ref.shape == rec.shape and np.array_equal(ref, rec), "oracle != generator reconstruction"
    assert ref_pocs == pocs, "PicOrderCnt"
    gold = json.load(open(GOLDEN))[name]
    assert hashlib.md5(stream).hexdigest() == gold["stream_md5"] and hashlib.md5(rec.tobytes()).hexdigest() == gold["frames_md5"] and pocs == gold["pocs"]


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipe_reaches_its_values(name, sg, oracle_mod):
    """What the generator counted while it built the prediction of this recipe (never in its motion search)."""
    ranges = _case(sg, oracle_mod, name)[3]
    print(name, {k: v for k, v in ranges.items() if v and abs(v) != 1 << 20})
    assert rangeutil.unmet(name, ranges, sg.SCALING_FORMS) == []


def test_golden_file_lists_the_recipes():
    assert set(json.load(open(GOLDEN))) == set(RECIPES)


def test_new_knobs_at_zero_change_nothing(sg):
    """wp_range, poc_step, mv_reach, mv_margin, contrast, dbf_per_slice and syntax_stim at 0 are today's streams, byte for byte (the golden files of the matrices show the same
    for every recipe there is); out-of-range settings of the knobs do not leave the generator's clamps."""
    kw = dict(width=64, height=48, frames=4, idr_period=0, profile_idc=77, cabac=1, weighted_pred=1, num_ref_frames=2, seed=5)
    a = sg.encode(**kw)[0]
    assert a == sg.encode(**dict(kw, wp_range=0, poc_step=0, mv_reach=0, mv_margin=0, contrast=0, dbf_per_slice=0, trace_deblock=0, syntax_stim=0))[0] == sg.encode(**dict(kw, poc_step=1))[0]
    assert sg.last_ranges()["scaling_forms"] == 0 and sg.last_ranges()["guard_zeroed"] == 0
    assert sg.last_deblock_trace() == []
    for k in ("wp_range", "poc_step", "mv_reach", "contrast", "dbf_per_slice", "syntax_stim"):
        assert a != sg.encode(**dict(kw, **{k: 2}))[0], k
    assert a != sg.encode(**dict(kw, syntax_stim=1))[0]
    # adding 4 only says which slices the syntax counters count; 3 is no stimulus
    assert sg.encode(**dict(kw, syntax_stim=1))[0] == sg.encode(**dict(kw, syntax_stim=5))[0] and a == sg.encode(**dict(kw, syntax_stim=3))[0]
    # the deblocking trace is a record, not a knob: the same stream and reconstruction with it, one entry per picture
    b, rec, _ = sg.encode(**dict(kw, trace_deblock=1))
    assert a == b and np.array_equal(rec, sg.encode(**kw)[1]) and sg.last_deblock_trace() == []


def _decode(H, streams, kws, x_wgs):
    from test_gpu_parity import _decode_gpu
    cfg = {}
    for kw in kws:
        cfg.update(decoder_cfg(kw))
    return _decode_gpu(H, streams, max(kw["width"] for kw in kws), max(kw["height"] for kw in kws), max(pictures_of(kw) for kw in kws),
                       max(kw.get("slices", 1) for kw in kws), x_wgs=x_wgs, **cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RECIPES))
def test_gpu_equals_generator_and_oracle(name, H, sg, oracle_mod):
    kw = RECIPES[name]
    stream, rec, pocs, _, ref, ref_pocs, _ = _case(sg, oracle_mod, name)
    gold = json.load(open(GOLDEN))[name]
    for x_wgs in (None, 0):  # the banded kernels of K3 / K5, and a picture inside one workgroup
        out, info = _decode(H, [stream], [kw], x_wgs)
        assert info.n_frames == kw["frames"]
        assert out[0].shape == rec.shape
        assert np.array_equal(out[0], rec), ("GPU != generator reconstruction", x_wgs, [i for i in range(len(rec)) if not np.array_equal(out[0][i], rec[i])])
        assert np.array_equal(out[0], ref), ("GPU != oracle", x_wgs)
        assert hashlib.md5(out[0].tobytes()).hexdigest() == gold["frames_md5"]
        assert info.pocs[0] == pocs == ref_pocs == gold["pocs"], "PicOrderCnt"


@pytest.mark.gpu
def test_gpu_batch_of_four_recipes(H, sg, oracle_mod):
    """A weighted stream, a far-vector stream and two streams under different PPS matrices in ONE batch: weights, vectors and scaling sets are per slice /
    per picture state of the launches they share."""
    names = ["wp2_b_pyramid_cabac", "mv_far_wide_cabac_p", "sm3_p_cabac", "sm3_b_cavlc"]
    cases = [_case(sg, oracle_mod, n) for n in names]
    for x_wgs in (None, 0):
        out, info = _decode(H, [c[0] for c in cases], [RECIPES[n] for n in names], x_wgs)
        for i, n in enumerate(names):
            kw = RECIPES[n]
            W, Hc = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
            assert info.pocs[i] == cases[i][2], (n, "PicOrderCnt")
            assert out[i].shape[0] == kw["frames"], n
            # the decoder's planes have the stream's own coded size
            assert np.array_equal(out[i][:, :W * Hc * 3 // 2], cases[i][1]), (n, x_wgs)


@pytest.mark.gpu
def test_gpu_more_scaling_matrices_than_sets(H, sg):
    """Every IDR picture of these streams brings an SPS with a new matrix: 12 distinct LevelScale sets in one batch, and 48 over the four batches of
    one decoder -- more than its table holds (32), so sets of finished batches must be given to new matrices, and the sets of the batch before
    must not be."""
    kws = [dict(width=48, height=32, frames=12, idr_period=1, profile_idc=100, cabac=k & 1, transform8x8=1, scaling_matrix=2, qp=20 + 6 * k, seed=200 + k) for k in range(4)]
    cases = [sg.encode(**kw) for kw in kws]
    assert len({c[0][:200] for c in cases}) == 4
    from test_gpu_parity import _x_wgs
    for x_wgs in (None, 0):
        with _x_wgs(x_wgs):
            dec = H.Decoder(max_streams=1, max_width=48, max_height=32, max_frames_per_batch=12, max_slices_per_frame=1)
            try:
                for k, (stream, rec, _) in enumerate(cases + cases[:1]):
                    dec.decode([stream])
                    assert np.array_equal(dec.read_frames(0, crop=False), rec), (k, x_wgs)
            finally:
                dec.close()


@pytest.mark.gpu
def test_gpu_scaling_sets_survive_batch_boundaries(H, sg, oracle_mod):
    """A stream whose every IDR picture brings a new SPS / PPS matrix, cut at access units into three decode() calls: the parameter sets and the scaling
    sets made from them must still be in force for the pictures of the next call."""
    name = "sm3_b_cavlc"
    kw = RECIPES[name]
    stream, rec, pocs, _, _, _, sizes = _case(sg, oracle_mod, name)
    ends = np.cumsum(sizes)
    assert int(ends[-1]) == len(stream)
    cuts = [0, int(ends[2]), int(ends[6]), len(stream)]  # (not at IDR pictures: the second and third part start under parameter sets of the part before)
    from test_gpu_parity import _x_wgs
    for x_wgs in (None, 0):
        with _x_wgs(x_wgs):
            dec = H.Decoder(max_streams=1, max_width=64, max_height=48, max_frames_per_batch=kw["frames"], max_slices_per_frame=1, b_pictures=1)
            try:
                got, got_pocs = [], []
                for a, b in zip(cuts, cuts[1:]):
                    dec.decode([stream[a:b]])
                    for f in range(dec.frame_count(0)):
                        got.append(dec.read_frame_tight(0, f, crop=False))
                        got_pocs.append(dec.frame_info(0, f).pic_order_cnt)
            finally:
                dec.close()
        assert got_pocs == pocs, x_wgs
        assert np.array_equal(np.stack(got), rec), ("GPU != generator reconstruction", x_wgs)
