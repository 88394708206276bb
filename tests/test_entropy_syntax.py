"""The entropy stage at the ends of its syntax (recipes: tests/syntaxutil.py): every entry of the coeff_token, total_zeros and run_before tables, level_prefix
14, 15 and the escape of 9.2.2.1 at every suffixLength, CABAC levels with long Exp-Golomb suffixes and saturated context counters, blocks that end at the last
scan position, every coded_block_flag increment, mb_qp_delta out to -26 / +25 and around the wrap of QP_Y, all coded_block_pattern and Intra16x16 mb_type
values, skip runs longer than a macroblock row and slices that end in a run or in I_PCM -- for I / P, B and field pictures and both entropy modes.
Generator, oracle and product are three separately written implementations; all three must agree bit for bit, and the generator's own counters (taken
where it writes the stream, never where it draws) must show that each recipe really goes where it claims to.  There is no tolerance anywhere in this file."""
import hashlib
import json
import os

import numpy as np
import pytest

import syntaxutil
from syntaxutil import BATCH_OF_FOUR, CABAC_IP_ROUTED, DENSEST, FAMILIES, FAMILY_OF, RECIPES, decoder_cfg, pictures_of, slices_of

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "entropy_syntax_md5.json")
_cache = {}


def _case(sg, oracle_mod, name):
    """(stream, generator reconstruction, generator PicOrderCnt, syntax counters, range counters, oracle frames, oracle PicOrderCnt, access unit sizes) of a
    recipe: made once, not modified"""
    if name not in _cache:
        stream, rec, sizes = sg.encode(**RECIPES[name])
        pocs, syn, ranges = [int(x) for x in sg.last_pocs()], sg.last_syntax(), sg.last_ranges()
        ref, _ = oracle_mod.decode(stream, crop=False)
        for a in (rec, ref):
            a.setflags(write=False)
        _cache[name] = (stream, rec, pocs, syn, ranges, ref, [int(x) for x in oracle_mod.last_pocs], sizes)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_oracle_equals_generator(name, sg, oracle_mod):
    stream, rec, pocs, _, _, ref, ref_pocs, _ = _case(sg, oracle_mod, name)
    assert ref.shape == rec.shape and np.array_equal(ref, rec), "oracle != generator reconstruction"
    assert ref_pocs == pocs, "PicOrderCnt"
    gold = json.load(open(GOLDEN))[name]
    assert hashlib.md5(stream).hexdigest() == gold["stream_md5"] and hashlib.md5(rec.tobytes()).hexdigest() == gold["frames_md5"] and pocs == gold["pocs"]


def _show(c):
    """the counters that are set; bitmaps and tables in hexadecimal"""
    out = []
    for k, v in c.items():
        if isinstance(v, list):
            if any(v):
                out.append("%s=[%s]" % (k, " ".join("%x" % x for x in v)))
        elif v and abs(v) != 1 << 20:
            out.append("%s=%s" % (k, "%#x" % v if k in syntaxutil.BITMAPS else v))
    return " ".join(out)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipe_reaches_its_syntax(name, sg, oracle_mod):
    """What the generator's entropy writers counted for this recipe and for its family (bitmaps in hexadecimal)."""
    family = {n: _case(sg, oracle_mod, n)[3] for n in FAMILIES[FAMILY_OF[name]]}
    print(name, "guard_zeroed=%d" % _case(sg, oracle_mod, name)[4]["guard_zeroed"], _show(family[name]))
    print("family", FAMILY_OF[name], _show(syntaxutil.union(family.values())))
    assert syntaxutil.unmet(name, family[name], family) == []


def test_golden_file_lists_the_recipes():
    assert set(json.load(open(GOLDEN))) == set(RECIPES)


def test_recipes_keep_to_their_limits():
    """pictures of 48x32 .. 96x80, at most 8 frames; one recipe at least for every row of the issue's table"""
    for name, kw in RECIPES.items():
        assert 48 <= kw["width"] <= 96 and 32 <= kw["height"] <= 80 and kw["frames"] <= 8 and kw["syntax_stim"] & 3, name
    have = lambda **want: any(all(kw.get(k, 0) == v for k, v in want.items()) for kw in RECIPES.values())
    assert have(profile_idc=66, cabac=0, slices=3) and have(profile_idc=100, cabac=0, transform8x8=1) and have(profile_idc=77, cabac=1, bframes=0, field_pics=0)
    assert have(profile_idc=100, cabac=1, transform8x8=1, bframes=0, field_pics=0) and have(bframes=3, cabac=0) and have(bframes=3, cabac=1)
    assert have(field_pics=1, cabac=0) and have(field_pics=1, cabac=1) and have(profile_idc=66, slice_groups=3) and have(mono=1)
    assert have(qp=0, chroma_qp_offset=-12) and have(qp=26) and have(qp=51, chroma_qp_offset=12) and have(skip_permille=900, pcm_permille=100, slices=3)


def _parse_level(bits, suffix_len, minus2):
    """9.2.2.1 as the standard states it, for the decoder: the level of one (level_prefix, level_suffix) pair, and the bits it took."""
    prefix = bits.index("1")
    size = 4 if prefix == 14 and suffix_len == 0 else (prefix - 3 if prefix >= 15 else suffix_len)
    suffix = int(bits[prefix + 1:prefix + 1 + size], 2) if size else 0
    code = (min(15, prefix) << suffix_len) + suffix
    if prefix >= 15 and suffix_len == 0:
        code += 15
    if prefix >= 16:
        code += (1 << (prefix - 3)) - 4096
    if minus2:
        code += 2
    return ((code + 2) >> 1 if code % 2 == 0 else (-code - 1) >> 1), prefix + 1 + size, prefix


def test_level_writer_against_the_rule_of_9_2_2_1(sg):
    """The generator's level writer, escape included, against the rule above -- not against one of the two decoders, which state the escape in the same
    words.  |level| 1..8200, every suffixLength, both cases of the first level after fewer than three trailing ones."""
    top = 0
    for suffix_len in range(7):
        for minus2 in (0, 1):
            for mag in range(1, 8201):
                for level in (mag, -mag):
                    if minus2 and mag == 1:
                        continue  # (such a level would have been a trailing one)
                    bits = sg.cavlc_level_bits(level, suffix_len, minus2)
                    assert bits is not None, (level, suffix_len, minus2)
                    got, used, prefix = _parse_level(bits, suffix_len, minus2)
                    assert (got, used) == (level, len(bits)), (level, suffix_len, minus2, bits)
                    top = max(top, prefix)
                    # Baseline / Main / Extended: nothing that needs level_prefix 16 is written
                    assert (sg.cavlc_level_bits(level, suffix_len, minus2, 0) is None) == (prefix > 15), (level, suffix_len, minus2)
    assert top == 17  # (8200 at suffixLength 0: levelCode 16398 = 30 + 4096 + 8192 + 4080)
    assert sg.cavlc_level_bits(2063, 0, 0, 0) is not None and sg.cavlc_level_bits(-2063, 1, 0, 0) is not None and sg.cavlc_level_bits(2064, 0, 0, 0) is None


def _decode(H, streams, kws, x_wgs, **more):
    from test_gpu_parity import _decode_gpu
    cfg = dict(more)
    for kw in kws:
        cfg.update(decoder_cfg(kw))
    return _decode_gpu(H, streams, max(kw["width"] for kw in kws), max(kw["height"] for kw in kws), max(pictures_of(kw) for kw in kws),
                       max(slices_of(kw) for kw in kws), x_wgs=x_wgs, **cfg)


def _status(H, streams, kws, x_wgs):
    """stream_status of every stream of a batch (a decoder of its own: _decode_gpu closes the one it makes)"""
    from test_gpu_parity import _x_wgs
    cfg = {}
    for kw in kws:
        cfg.update(decoder_cfg(kw))
    with _x_wgs(x_wgs):
        dec = H.Decoder(max_streams=len(streams), max_width=max((kw["width"] + 15) & ~15 for kw in kws), max_height=max((kw["height"] + 15) & ~15 for kw in kws),
                        max_frames_per_batch=max(pictures_of(kw) for kw in kws), max_slices_per_frame=max(slices_of(kw) for kw in kws), **cfg)
        try:
            dec.decode(streams)
            return [dec.stream_status(i) for i in range(len(streams))], [dec.read_frames(i, crop=False) for i in range(len(streams))]
        finally:
            dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RECIPES))
def test_gpu_equals_generator_and_oracle(name, H, sg, oracle_mod):
    kw = RECIPES[name]
    stream, rec, pocs, _, _, ref, ref_pocs, _ = _case(sg, oracle_mod, name)
    gold = json.load(open(GOLDEN))[name]
    for x_wgs in (None, 0):  # the banded kernels of K3 / K5, and a picture inside one workgroup
        out, info = _decode(H, [stream], [kw], x_wgs)
        assert info.n_frames == kw["frames"]
        assert out[0].shape == rec.shape
        assert np.array_equal(out[0], rec), ("GPU != generator reconstruction", x_wgs, [i for i in range(len(rec)) if not np.array_equal(out[0][i], rec[i])])
        assert np.array_equal(out[0], ref), ("GPU != oracle", x_wgs)
        assert hashlib.md5(out[0].tobytes()).hexdigest() == gold["frames_md5"]
        assert info.pocs[0] == pocs == ref_pocs == gold["pocs"], "PicOrderCnt"
    status, frames = _status(H, [stream], [kw], None)
    assert status == [0] and np.array_equal(frames[0], rec)


def _small_cavlc(sg):
    if "small_cavlc" not in _cache:
        kw = dict(width=48, height=32, frames=3, idr_period=0, profile_idc=66, cabac=0, seed=77)
        stream, rec, _ = sg.encode(**kw)
        rec.setflags(write=False)
        _cache["small_cavlc"] = (kw, stream, rec)
    return _cache["small_cavlc"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CABAC_IP_ROUTED)
def test_gpu_cabac_recipe_next_to_a_cavlc_stream(name, H, sg, oracle_mod):
    """An I / P CABAC stream alone takes k_entropy_c (test_gpu_equals_generator_and_oracle); next to a CAVLC stream in the same batch its slices share
    launches with CAVLC slices and take the CABAC path of k_entropy.  Both must be exact."""
    kw = RECIPES[name]
    stream, rec = _case(sg, oracle_mod, name)[:2]
    kw2, stream2, rec2 = _small_cavlc(sg)
    for x_wgs in (None, 0):
        status, frames = _status(H, [stream, stream2], [kw, kw2], x_wgs)
        assert status == [0, 0], x_wgs
        W, Hc = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
        assert np.array_equal(frames[0][:, :W * Hc * 3 // 2], rec), (name, x_wgs)
        assert np.array_equal(frames[1][:, :48 * 32 * 3 // 2], rec2), ("the CAVLC stream", x_wgs)


@pytest.mark.gpu
def test_gpu_batch_of_four_families(H, sg, oracle_mod):
    """A CAVLC High stream with escape-coded levels, a CABAC stream with large levels, a QP-wrap stream and a skip / I_PCM stream in ONE batch: levels, QP_Y
    and the skip state are per slice state of the launches they share."""
    assert [FAMILY_OF[n] for n in BATCH_OF_FOUR] == ["cavlc_ip", "cabac_ip", "qp", "skip_pcm"]
    cases = [_case(sg, oracle_mod, n) for n in BATCH_OF_FOUR]
    assert cases[0][3]["prefix_max"] >= 16 and cases[1][3]["egk_max"] >= 11 and cases[2][3]["dqp_wrap_up"] and cases[2][3]["dqp_wrap_down"] and cases[3][3]["end_in_skip"]
    for x_wgs in (None, 0):
        out, info = _decode(H, [c[0] for c in cases], [RECIPES[n] for n in BATCH_OF_FOUR], x_wgs)
        for i, n in enumerate(BATCH_OF_FOUR):
            kw = RECIPES[n]
            W, Hc = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
            assert info.pocs[i] == cases[i][2], (n, "PicOrderCnt")
            assert out[i].shape[0] == kw["frames"], n
            assert np.array_equal(out[i][:, :W * Hc * 3 // 2], cases[i][1]), (n, x_wgs)


@pytest.mark.gpu
def test_gpu_densest_recipe_in_three_calls_with_a_sized_pool(H, sg, oracle_mod):
    """The recipe with the most residual per macroblock, cut at access units into three decode() calls, on a decoder whose residual pool is the smallest that
    h264mi_config.coef_blocks_per_mb can make and that still holds what the stream needs (as a roomy decoder reports it): full blocks with large levels
    are not taken for an exhausted pool -- no pass is repeated, no stream is marked -- and the pictures are exact."""
    name = DENSEST
    per_mb = {n: len(_case(sg, oracle_mod, n)[0]) / (RECIPES[n]["frames"] * ((RECIPES[n]["width"] + 15) // 16) * ((RECIPES[n]["height"] + 15) // 16)) for n in RECIPES
              if n not in syntaxutil.OVERSIZED}
    assert max(per_mb, key=per_mb.get) == name, per_mb
    kw = RECIPES[name]
    stream, rec, pocs, _, _, _, _, sizes = _case(sg, oracle_mod, name)
    ends = np.cumsum(sizes)
    assert int(ends[-1]) == len(stream)
    cuts = [0, int(ends[len(ends) // 3 - 1]), int(ends[2 * len(ends) // 3 - 1]), len(stream)]
    W, Hc, slices = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15, slices_of(kw)
    geometry = dict(max_streams=1, max_width=W, max_height=Hc, max_frames_per_batch=pictures_of(kw), max_slices_per_frame=slices, **decoder_cfg(kw))
    roomy = H.Decoder(**geometry)
    try:
        need = 0
        for a, b in zip(cuts, cuts[1:]):
            roomy.decode([stream[a:b]])
            need = max(need, roomy.coef_pool()[0])
    finally:
        roomy.close()
    # the pool of this geometry: coef_blocks_per_mb blocks for every macroblock record, and the chunk head-room of its slices
    caps = []
    for k in (1, 2):
        d = H.Decoder(coef_blocks_per_mb=k, **geometry)
        caps.append(d.coef_pool()[1])
        d.close()
    per_k, head = caps[1] - caps[0], 2 * caps[0] - caps[1]
    assert per_k > 0 and head > 0, caps
    k = max(1, -(-(need - head) // per_k))
    assert k <= 26, (need, caps)  # (26 blocks per macroblock are the worst case of the syntax)
    from test_gpu_parity import _x_wgs
    for x_wgs in (None, 0):
        with _x_wgs(x_wgs):
            dec = H.Decoder(coef_blocks_per_mb=k, **geometry)
            try:
                got, got_pocs = [], []
                for a, b in zip(cuts, cuts[1:]):
                    dec.decode([stream[a:b]])
                    used, cap = dec.coef_pool()
                    assert 0 < used <= cap, (used, cap, k)
                    assert dec.stream_status(0) == 0
                    for f in range(dec.frame_count(0)):
                        got.append(dec.read_frame_tight(0, f, crop=False))
                        got_pocs.append(dec.frame_info(0, f).pic_order_cnt)
            finally:
                dec.close()
        assert got_pocs == pocs, x_wgs
        assert np.array_equal(np.stack(got), rec), ("GPU != generator reconstruction", x_wgs)
