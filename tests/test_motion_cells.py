"""Motion vector derivation (8.4.1) cell by cell on whole streams (recipes and yardstick: tests/motionutil.py).  A cell is the rule that decided one
derivation: which clause of 8.4.1.3 gave the predictor and where neighbour C came from, which condition of P_Skip held, which neighbour gave a spatial
direct index, the factors of colZeroFlag, what the co-located block was, how temporal direct mapped and scaled it.

On the CPU: the generator's final vectors and reference indices against the plain-Python yardstick applied to the generator's own motion trace (the
syntax as written and the slices' lists) -- a fourth writing of 8.4.1, independent of generator, oracle and product --; the oracle's vectors and
indices for all sixteen blocks and both lists against the same field; the oracle's frames against the generator's, the golden MD5s, and the cells
each recipe reaches, counted by the yardstick.  The set of reachable cells is enumerated from the rules; the recipes together must reach it, within
the exemptions motionutil names.

On the GPU: the per-4x4 motion field of Decoder.side_info against the yardstick's on every block, and the frames against generator, oracle and golden
MD5: every P CABAC recipe on k_entropy_m, k_entropy_c and k_entropy, B and slice-group recipes on k_entropy_b, four unlike recipes in one batch.  There
is no tolerance anywhere in this file."""
import hashlib
import json
import os

import numpy as np
import pytest

import motionutil as M
from motionutil import B_RECIPES, FMO_RECIPES, GEOMETRY, P_RECIPES, RECIPES

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "motion_md5.json")
COUNTERS_TXT = os.path.join(os.path.dirname(__file__), "golden", "motion_counters.txt")
_cache = {}


def _case(sg, oracle_mod, name):
    """(stream, generator reconstruction, motion trace, the yardstick's pictures, oracle frames, oracle motion trace, the generator's motion counters) of a
    recipe: made once, not modified"""
    if name not in _cache:
        kw = RECIPES[name]
        stream, rec, _ = sg.encode(**kw)
        trace, counters = sg.last_motion_trace(), sg.last_motion()
        pics = M.derive_stream(trace, inference=not kw.get("direct_4x4"))
        ref, _, motion = oracle_mod.decode(stream, crop=False, motion=True)
        for a in (rec, ref, motion):
            a.setflags(write=False)
        _cache[name] = (stream, rec, trace, pics, ref, motion, counters)
    return _cache[name]


def _cells(pics):
    total = M.Counter()
    for p in pics:
        total.update(p.cells)
    return total


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_yardstick_equals_generator(name, sg, oracle_mod):
    """the independent pin: 8.4.1 in plain Python from the syntax as written gives the generator's final vector for every list and 4x4 block and its
    reference index for every list and quadrant"""
    kw = RECIPES[name]
    _, _, trace, pics, _, _, _ = _case(sg, oracle_mod, name)
    assert len(trace) == kw["frames"] == len(pics) and all(t["field"] == 0 for t in trace)
    diff = M.first_difference(pics, trace)
    assert diff is None, ("yardstick != generator: (picture, macroblock, list, what, block / quadrant, yardstick, generator)", name, diff)
    # the trace is not empty-handed: inter macroblocks, and in B recipes both lists and direct macroblocks
    kinds = np.concatenate([t["mbs"]["kind"].reshape(-1) for t in trace])
    assert (kinds == M.KIND_INTRA).any() and ((kinds >= M.KIND_16x16) & (kinds <= M.KIND_8x8)).any()
    if M.is_b(kw):
        assert any((t["mbs"]["ref"][:, :, 1] >= 0).any() for t in trace) and (kinds >= M.KIND_BDIRECT).any()
        assert any(int(s["col_index"]) >= 0 for t in trace for s in t["slices"] if s["type"] == M.SLICE_B)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_oracle_motion_equals_yardstick(name, sg, oracle_mod):
    """the oracle's macroblock trace, all sixteen blocks and both lists, in its own decoding order"""
    _, _, trace, pics, _, motion, _ = _case(sg, oracle_mod, name)
    assert len(motion) == sum(p.hmb * p.wmb for p in pics)
    for row in motion:
        addr, pic_no = int(row[0]), int(row[2])
        p = pics[pic_no]
        ref = row[68:76].reshape(2, 4)
        used = np.repeat(np.repeat(ref.reshape(2, 2, 2) >= 0, 2, axis=1), 2, axis=2).reshape(2, 16)
        # (per list: quadrant rows x quadrant columns -> the 4x4 blocks of each quadrant, in raster order)
        mv = np.where(used[:, :, None], row[4:68].reshape(2, 16, 2), 0)
        assert int(row[1]) == int(trace[pic_no]["slices"][int(p.slice_of[addr])]["type"]), ("slice type", name, pic_no, addr)
        assert np.array_equal(ref, p.ref[addr]), ("oracle != yardstick: reference indices", name, "picture", pic_no, "macroblock", addr, ref.tolist(), p.ref[addr].tolist())
        bad = np.argwhere((mv != p.mv[addr]).any(axis=2))
        assert not len(bad), ("oracle != yardstick: vectors (list, block)", name, "picture", pic_no, "macroblock", addr, bad[0].tolist(),
                              mv[tuple(bad[0])].tolist(), p.mv[addr][tuple(bad[0])].tolist())


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_oracle_equals_generator(name, sg, oracle_mod):
    stream, rec, _, _, ref, _, _ = _case(sg, oracle_mod, name)
    assert ref.shape == rec.shape and np.array_equal(ref, rec), "oracle != generator reconstruction"
    gold = json.load(open(GOLDEN))[name]
    assert hashlib.md5(stream).hexdigest() == gold["stream_md5"] and hashlib.md5(rec.tobytes()).hexdigest() == gold["frames_md5"]
    plain = dict(RECIPES[name], trace_motion=0)
    assert sg.encode(want_recon=False, **plain)[0] == stream, "trace_motion changed the stream"


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipe_reaches_its_cells(name, sg, oracle_mod):
    """what the yardstick counted on this recipe's trace: nothing the enumeration calls unreachable, and the line of the golden file"""
    cells = _cells(_case(sg, oracle_mod, name)[3])
    print(M.cell_line(name, cells))
    assert M.beyond_reach(cells) == []
    assert M.cell_line(name, cells) in open(COUNTERS_TXT).read().split("\n")


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_generator_counts_what_the_yardstick_counts(name, sg, oracle_mod):
    """the generator's own counters (SG_M_*: counted in mv_pred / mv_pred_l, skip_mv and b_direct, where the predictor that goes into the stream is built, and
    in the entropy writers) against the cells the yardstick counted from the trace: equal, cell by cell; every enumerated cell has a word of the generator's,
    and the writers' words about ref_idx, mvd, mb_skip_flag and the first bin of a B mb_type are counted again from the trace and must be equal too"""
    case = _case(sg, oracle_mod, name)
    cells, g = _cells(case[3]), case[6]
    differ = {k: (v, cells.get(k, 0)) for k, v in g.items() if isinstance(k, tuple) and v != cells.get(k, 0)}
    assert not differ, ("generator's counters != the yardstick's (generator, yardstick)", differ)
    assert all(k in M.reachable_cells() for k, v in g.items() if isinstance(k, tuple) and v), "the generator counted what the enumeration calls unreachable"
    for st, word, cell in (("P", "mbtype_p", "mb_type"), ("B", "mbtype_b", "mb_type"), ("P", "subtype_p", "sub_mb_type"), ("B", "subtype_b", "sub_mb_type")):
        assert g[word] == sum(1 << k[2] for k in cells if k[0] == cell and k[1] == st), word
    # every enumerated cell has a word of the generator's behind it (mb_type and sub_mb_type: the four masks above)
    assert all(c in g for c in M.reachable_cells() if c[0] not in ("mb_type", "sub_mb_type"))
    # ... and what the entropy writers counted about ref_idx, mvd, mb_skip_flag and the first bin of a B mb_type, counted again from the trace
    syntax = dict.fromkeys(M.SYNTAX_MASKS + M.SYNTAX_COUNTS, 0)
    for p in case[3]:
        for k, v in M.count_syntax(p, RECIPES[name]["cabac"]).items():
            syntax[k] = syntax[k] | v if k in M.SYNTAX_MASKS else syntax[k] + v
    differ = {k: (g[k], v) for k, v in syntax.items() if g[k] != v}
    assert not differ, ("the writers' counters != the yardstick's recount (generator, yardstick)", differ)
    assert set(syntax) | {"mbtype_p", "mbtype_b", "subtype_p", "subtype_b"} == {k for k in g if isinstance(k, str)}, "a word of the writers' that nothing recounts"


def test_recipes_reach_the_motion_syntax(sg, oracle_mod):
    """what only the entropy writers can say, over all recipes: every mb_type and sub_mb_type, the four first-bin increments of ref_idx, an index of at
    least 3, a direct or skipped neighbour counted as index 0, te() in its one-bit form and as ue(), the three context bands of mvd per component, a
    prefix of nine ones with a suffix, the three increments of mb_skip_flag in P and in B slices and of the first bin of a B mb_type"""
    total = {}
    for name in RECIPES:
        for k, v in _case(sg, oracle_mod, name)[6].items():
            if isinstance(k, str):
                total[k] = total.get(k, 0) | v if k.endswith(("_p", "_b", "_inc")) else total.get(k, 0) + v
    assert total["mbtype_p"] == 0x1F and total["mbtype_b"] == (1 << 23) - 1 and total["subtype_p"] == 0xF and total["subtype_b"] == (1 << 13) - 1
    assert total["ref_inc"] == 0xF and total["skip_inc_p"] == 7 and total["skip_inc_b"] == 7 and total["btype_inc"] == 7
    for k in ("ref_ge3", "ref_direct_nb", "ref_te1", "ref_ue", "mvd_suffix") + tuple("mvd_band_%s_%d" % (c, b) for c in "xy" for b in range(3)):
        assert total[k] > 0, k


def test_every_reachable_cell_is_reached_by_a_recipe(sg, oracle_mod):
    """the union of what the recipes reach is the enumeration of what can be reached, but for the cells exempted by name -- at most one in twenty of a
    family, none of the P_Skip, co-located and temporal families"""
    total = M.Counter()
    for name in RECIPES:
        total.update(_cells(_case(sg, oracle_mod, name)[3]))
    reach = M.reachable_cells()
    missing = sorted((c for c in reach if c not in total), key=repr)
    print("reachable", len(reach), "reached", len(M.counted(total)), "missing", missing)
    assert M.beyond_reach(total) == []
    assert sorted(M.EXEMPT, key=repr) == missing, "the cells no recipe reaches are exactly the ones exempted by name"
    assert all(isinstance(why, str) and why and "\n" not in why for why in M.EXEMPT.values())
    for family in set(M.FAMILY.values()):
        n = sum(1 for c in reach if M.FAMILY[c[0]] == family)
        ex = sum(1 for c in M.EXEMPT if M.FAMILY[c[0]] == family)
        assert ex * 20 <= n and not (ex and family in M.NO_EXEMPTION), (family, ex, n)


def test_enumeration_has_the_shape_the_rules_give():
    reach = M.reachable_cells()
    assert len({c for c in reach if c[0] == "geo"} | set()) >= 41 and {c[1] for c in reach if c[0] == "geo"} == set(range(41))
    assert sum(1 for c in reach if c[0] == "pskip") == 6
    assert sum(1 for c in reach if c[0] == "mb_type") == 5 + 23 and sum(1 for c in reach if c[0] == "sub_mb_type") == 4 + 13
    # the partitions whose C lies inside the macroblock, counted by hand: 8x8: quadrant 2 (C in quadrant 1, there); 8x4: the lower one of quadrant 0
    # (C in quadrant 1, not yet), both of quadrant 2 (quadrant 1: there; quadrant 3: not yet); 4x8: both of quadrant 2 and the left one of quadrant 3
    # (all there); 4x4: nine, of which the last of quadrant 0 and of quadrant 2 look into a later quadrant.  16 in all, 4 of them "not yet"
    inside = {c[1]: c[2] for c in reach if c[0] == "geo" and c[2] in ("in_done", "in_later")}
    assert len(inside) == 16 and sum(1 for v in inside.values() if v == "in_later") == 4
    assert ("pred", "P", 0, "16x8l", "onlyA") not in reach and ("pred", "B", 1, "med", "med3") in reach


def test_golden_file_lists_the_recipes():
    assert set(json.load(open(GOLDEN))) == set(RECIPES)
    lines = [ln for ln in open(COUNTERS_TXT).read().split("\n") if ln.startswith("  ")]
    assert sorted(ln.split()[0] for ln in lines) == sorted(RECIPES)


def test_new_knobs_at_zero_change_nothing(sg):
    """direct_4x4, trace_motion and motion_stim at 0 are today's streams, byte for byte (the golden files of the matrices show the same for every recipe there is); the
    trace is a record, not a knob; direct_4x4 is refused where the SPS could not carry it"""
    kw = dict(width=64, height=48, frames=7, idr_period=0, profile_idc=100, cabac=1, transform8x8=1, bframes=2, num_ref_frames=3, bskip_permille=150,
              sub8x8_permille=400, seed=5)
    a, rec, _ = sg.encode(**kw)
    assert a == sg.encode(**dict(kw, direct_4x4=0, trace_motion=0, motion_stim=0))[0] and sg.last_motion_trace() == []
    assert a != sg.encode(**dict(kw, motion_stim=1))[0]
    assert a == sg.encode(**dict(kw, motion_stim=2))[0], "only 1 is a stimulus"
    b, rec_b, _ = sg.encode(**dict(kw, trace_motion=1))
    assert a == b and np.array_equal(rec, rec_b) and len(sg.last_motion_trace()) == 7
    c = sg.encode(**dict(kw, direct_4x4=1))[0]
    assert c != a
    for bad in (dict(field_pics=1), dict(interlace_sps=1)):
        with pytest.raises(RuntimeError, match="direct_4x4"):
            sg.encode(**dict(kw, direct_4x4=1, height=64, **bad))


def test_recipes_cover_what_the_issue_names():
    """the options and sizes the recipes switch on, so that a recipe edited later cannot quietly lose one"""
    for kw in list(P_RECIPES.values()) + list(B_RECIPES.values()) + list(FMO_RECIPES.values()):
        assert 48 <= kw["width"] <= 96 and 32 <= kw["height"] <= 80 and kw["frames"] <= 8 and kw["trace_motion"] == 1, kw
    ps = list(P_RECIPES.values())
    for cabac in (0, 1):
        mine = [k for k in ps if k["cabac"] == cabac]
        assert {k["num_ref_frames"] for k in mine} >= {1, 3} and any(k.get("slices") == 3 and k.get("intra_stim") == 1 for k in mine)
        assert any(k.get("slices", 1) == 1 for k in mine)
    assert any(k["intra_in_p_permille"] >= 300 for k in ps) and any(k["sub8x8_permille"] >= 800 for k in ps)
    bs = list(B_RECIPES.values())
    for temporal in (0, 1):
        for d4 in (0, 1):
            assert any(k.get("direct_temporal", 0) == temporal and k.get("direct_4x4", 0) == d4 for k in bs), (temporal, d4)
    assert {k["cabac"] for k in bs} == {0, 1}
    assert any(k.get("transform8x8") and k.get("direct_4x4") for k in bs) and any(k.get("transform8x8") and not k.get("direct_4x4") for k in bs)
    assert any(not k.get("transform8x8") for k in bs) and any(k.get("b_pyramid") and k.get("direct_temporal") for k in bs)
    assert any(k.get("slice_groups", 0) > 1 and not M.is_b(k) for k in FMO_RECIPES.values())
    assert sorted((k["width"], k["height"]) for k in GEOMETRY.values() if not M.is_b(k)) == sorted([(16, 16), (176, 16), (16, 144), (32, 32), (176, 144)])
    assert all(k["frames"] == 4 and k["width"] <= 176 and k["height"] <= 144 for k in GEOMETRY.values())


def test_a_wrong_rule_in_the_yardstick_is_noticed(sg, oracle_mod, monkeypatch):
    """the comparison has teeth: the median replaced by the mean, DistScaleFactor off by one, the corner substitution left out -- each is found"""
    trace = _case(sg, oracle_mod, "p_cabac_sub_heavy")[2]
    assert M.first_difference(M.derive_stream(trace), trace) is None
    monkeypatch.setattr(M, "_median", lambda a, b, c: (a + b + c) // 3)
    assert M.first_difference(M.derive_stream(trace), trace) is not None
    monkeypatch.undo()
    trace_t = _case(sg, oracle_mod, "b_temporal_cabac")[2]
    monkeypatch.setattr(M, "_idiv", lambda a, b: a // b)          # "/" that rounds down instead of towards zero
    monkeypatch.setattr(M, "_clip3", lambda lo, hi, v: v + 1)
    assert M.first_difference(M.derive_stream(trace_t), trace_t) is not None
    monkeypatch.undo()
    trace_b = _case(sg, oracle_mod, "b_spatial_cabac")[2]
    assert M.first_difference(M.derive_stream(trace_b, inference=False), trace_b) is not None, "direct_8x8_inference_flag matters"


# ---- GPU ----
PLANES = ("type", "mvx0", "mvy0", "ref0", "mvx1", "mvy1", "ref1")
GENERAL, FMO, CABAC, MAIN = 0, 1, 2, 3   # h264mi_internal_entropy_kernel_choice4


def _decode_with_side(H, items):
    """items: [(kw, stream)] decoded as ONE batch; per stream (frames uncropped, the side-information planes of its frames as numpy [frame, plane, gh, gw])"""
    from test_entropy_main_gpu import _nslices
    W = max(kw["width"] for kw, _ in items)
    Hc = max(kw["height"] for kw, _ in items)
    dec = H.Decoder(max_streams=len(items), max_width=W, max_height=Hc, max_frames_per_batch=max(kw["frames"] for kw, _ in items),
                    max_slices_per_frame=max(_nslices(kw) for kw, _ in items), max_bitstream_bytes=sum(len(s) for _, s in items) * 2 + (1 << 20))
    try:
        dec.decode([s for _, s in items])
        out = []
        for i, (kw, _) in enumerate(items):
            frames = dec.read_frames(i, crop=True, size=kw["width"] * kw["height"] * 3 // 2)
            side = np.stack([v.cpu().numpy() for v in dec.side_info(stream=i, planes=PLANES)])
            out.append((frames, side))
        return out
    finally:
        dec.close()


def _type_plane(H, planes):
    """the "type" plane the yardstick's macroblock kinds ask for; -1 where the trace does not say which intra type it was"""
    kind, st = planes["kind"], planes["slice_type"]
    p_types = np.array([-1, H.MB_P16x16, H.MB_P16x8, H.MB_P8x16, H.MB_P8x8, H.MB_PSKIP, -2, -2])
    b_types = np.array([-1, H.MB_B, H.MB_B, H.MB_B, H.MB_B, -2, H.MB_BDIRECT, H.MB_BSKIP])
    return np.where(st == M.SLICE_B, b_types[kind], p_types[kind])


def _check(H, name, got, case, what):
    frames, side = got
    stream, rec, trace, pics, ref, _, _ = case
    assert frames.shape == rec.shape and np.array_equal(frames, rec), ("GPU != generator reconstruction", name, what)
    assert np.array_equal(frames, ref), ("GPU != oracle", name, what)
    assert hashlib.md5(frames.tobytes()).hexdigest() == json.load(open(GOLDEN))[name]["frames_md5"], (name, what)
    assert side.shape[0] == len(pics), (name, what)
    for t, p in zip(trace, pics):
        f, want = t["frame"], M.planes_of(p)
        assert side[f].shape[1:] == want["ref0"].shape, (name, what)
        for i, plane in enumerate(PLANES[1:], 1):
            bad = np.argwhere(side[f][i] != want[plane])
            assert not len(bad), ("GPU != yardstick", name, what, "frame", f, plane, "first (block row, block column)", bad[0].tolist(),
                                  int(side[f][i][tuple(bad[0])]), int(want[plane][tuple(bad[0])]))
        types = _type_plane(H, want)
        assert not (types == -2).any()
        got_t = side[f][0]
        assert np.array_equal(np.where(types >= 0, got_t, -1), types) and ((got_t[types < 0] >= H.MB_I4x4) & (got_t[types < 0] <= H.MB_IPCM)).all(), ("type plane", name, what, f)


_P_MAIN = sorted(n for n, kw in RECIPES.items() if M.main_eligible(kw))
_B_OR_FMO = sorted(n for n, kw in RECIPES.items() if M.is_b(kw) or kw.get("slice_groups", 0) > 1)
_OTHER = sorted(set(RECIPES) - set(_P_MAIN) - set(_B_OR_FMO))


@pytest.mark.gpu
@pytest.mark.parametrize("name", _P_MAIN)
def test_gpu_p_cabac_field_on_three_routes(name, H, sg, oracle_mod):
    """alone on k_entropy_m, next to an 8x8-transform stream on k_entropy_c, next to a CAVLC stream on k_entropy"""
    from test_entropy_main_gpu import _route
    kw, case = RECIPES[name], _case(sg, oracle_mod, name)
    cav_kw = RECIPES["p_cavlc_1ref"]
    t8_kw = dict(width=48, height=32, frames=2, idr_period=1, profile_idc=100, cabac=1, transform8x8=1, seed=9)   # two I pictures with the 8x8 transform
    assert cav_kw["cabac"] == 0
    assert _route(H, [kw]) == MAIN and _route(H, [kw, t8_kw]) == CABAC and _route(H, [kw, cav_kw]) == GENERAL
    t8 = sg.encode(want_recon=False, **t8_kw)[0]
    cav = _case(sg, oracle_mod, "p_cavlc_1ref")
    _check(H, name, _decode_with_side(H, [(kw, case[0])])[0], case, "alone: k_entropy_m")
    _check(H, name, _decode_with_side(H, [(kw, case[0]), (t8_kw, t8)])[0], case, "next to an 8x8-transform stream: k_entropy_c")
    both = _decode_with_side(H, [(kw, case[0]), (cav_kw, cav[0])])
    _check(H, name, both[0], case, "next to a CAVLC stream: k_entropy")
    _check(H, "p_cavlc_1ref", both[1], cav, "the CAVLC stream of the mixed batch")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _B_OR_FMO + _OTHER)
def test_gpu_field_equals_yardstick(name, H, sg, oracle_mod):
    """B recipes (their B slices on k_entropy_b; their I and P pictures go where level 0 of the batch goes, which is not asserted here), the slice-group
    recipe (k_entropy_b, asserted), and the P recipes that are not eligible for k_entropy_m (CAVLC: k_entropy)"""
    from test_entropy_main_gpu import _route
    kw, case = RECIPES[name], _case(sg, oracle_mod, name)
    if kw.get("slice_groups", 0) > 1:
        assert _route(H, [kw]) == FMO
    _check(H, name, _decode_with_side(H, [(kw, case[0])])[0], case, "alone")


@pytest.mark.gpu
def test_gpu_batch_of_four_recipes(H, sg, oracle_mod):
    """P CAVLC, P CABAC, B spatial without direct_8x8_inference_flag and B temporal in ONE batch of one decoder"""
    names = ["p_cavlc_3ref_3slices_midrow", "p_cabac_3ref", "b_spatial_d4_cabac", "b_temporal_cabac"]
    kws = [RECIPES[n] for n in names]
    assert not kws[0]["cabac"] and kws[1]["cabac"] and kws[2].get("direct_4x4") and not kws[2].get("direct_temporal") and kws[3].get("direct_temporal")
    cases = [_case(sg, oracle_mod, n) for n in names]
    got = _decode_with_side(H, [(kw, c[0]) for kw, c in zip(kws, cases)])
    for n, g, c in zip(names, got, cases):
        _check(H, n, g, c, "batch of four")
