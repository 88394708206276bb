"""Residual decoding (8.5) cell by cell on whole streams (recipes and yardstick: tests/residualutil.py).  A cell is one decision of 8.5: the QPc a plane
got from which qPI, the branch and the qP a class of block was scaled with and the sign that met the rounding term, the scan position a level came from,
the scaling list a block used, the coded_block_pattern of a macroblock, the row pairs of an 8x8 block that hold coefficients, the planes that carry
chroma DC / AC, what K4 finds in the four macroblocks of a wavefront, and the values at which the arithmetic can go wrong.

On the CPU: the generator's picture before deblocking against the numpy yardstick applied to the generator's own residual trace (the prediction of every
sample and the levels as the entropy writer wrote them) -- a fourth writing of 8.5, independent of generator, oracle and product --; that picture,
deblocked by the yardstick of test_deblock_*.py, against the generator's reconstruction; the oracle's frames against the generator's, the golden MD5s,
and the cells each recipe reaches.  The set of reachable cells is enumerated from the rules; the recipes together must reach it, but for the exemptions
residualutil names.

On the GPU: every recipe through the banded K3 and through one workgroup per picture, against generator, oracle and golden MD5, a mismatch reported as
the first wrong macroblock with the yardstick's class words; the qp and nz planes of Decoder.side_info against the yardstick; every Main-eligible P CABAC
recipe on k_entropy_m, k_entropy_c and k_entropy; four unlike recipes in one batch.  There is no tolerance anywhere in this file."""
import hashlib
import json
import os

import numpy as np
import pytest

import deblockutil as D
import residualutil as R
from rangeutil import decoder_cfg, pictures_of
from residualutil import B_RECIPES, FIELD_RECIPES, GEOMETRY, I_RECIPES, MONO_RECIPES, P_RECIPES, RECIPES

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "residual_md5.json")
COUNTERS_TXT = os.path.join(os.path.dirname(__file__), "golden", "residual_counters.txt")
_cache = {}


def _case(sg, oracle_mod, name):
    """(stream, generator reconstruction, residual trace, the yardstick's pictures, oracle frames) of a recipe: made once, not modified"""
    if name not in _cache:
        stream, rec, _ = sg.encode(**RECIPES[name])
        trace = sg.last_residual_trace()
        pics = R.reconstruct_stream(trace)
        ref, _ = oracle_mod.decode(stream, crop=False)
        for a in (rec, ref):
            a.setflags(write=False)
        _cache[name] = (stream, rec, trace, pics, ref)
    return _cache[name]


def _cells(pics):
    total = R.Counter()
    for p in pics:
        total.update(p.cells)
    return total


def _frame_planes(frame, W, H):
    return frame[:W * H].reshape(H, W), frame[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), frame[W * H * 5 // 4:].reshape(H // 2, W // 2)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_yardstick_equals_generator(name, sg, oracle_mod):
    """the independent pin: 8.5 in numpy from the levels as written gives the generator's picture before deblocking, sample by sample; that picture,
    deblocked by the yardstick of 8.7, is the generator's reconstruction; QPc is the one the generator deblocks with"""
    kw = RECIPES[name]
    _, rec, trace, pics, _ = _case(sg, oracle_mod, name)
    W, H = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
    assert len(trace) == len(pics) and kw["frames"] <= len(trace) <= pictures_of(kw)
    assert len(trace) == pictures_of(kw) or kw.get("field_pics") == 3, "only a picture-adaptive stream has fewer pictures than fields"
    for i, (t, p) in enumerate(zip(trace, pics)):
        diff = R.first_difference(p, t["planes"])
        assert diff is None, ("yardstick != generator: (macroblock, plane, block, the block's class word, yardstick, generator)", name, "picture", i, diff)
        if not t["mono"]:
            assert np.array_equal(p.qpc, t["mbs"]["qpc"]), ("QPc", name, i, np.argwhere(p.qpc != t["mbs"]["qpc"])[:4].tolist())
        out = D.deblock_picture(p.planes, t["mbs"], t["field"] != 0, t["mono"])
        rows = slice(None) if t["field"] == 0 else slice(t["field"] - 1, None, 2)
        for plane, (got, whole) in enumerate(zip(out, _frame_planes(rec[t["frame"]], W, H))):
            if not (t["mono"] and plane):
                assert np.array_equal(whole[rows], got), ("yardstick, deblocked, != reconstruction", name, i, plane)
    # the trace is not empty-handed
    kinds = np.concatenate([t["rsmbs"]["kind"].reshape(-1) for t in trace])
    assert (kinds >= R.RS_I4).any() and any(t["rsmbs"]["luma"].any() for t in trace)
    if kw.get("idr_period", 1) != 1:
        assert (kinds == R.RS_INTER).any()


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_oracle_equals_generator(name, sg, oracle_mod):
    stream, rec, _, _, ref = _case(sg, oracle_mod, name)
    assert ref.shape == rec.shape and np.array_equal(ref, rec), "oracle != generator reconstruction"
    gold = json.load(open(GOLDEN))[name]
    assert hashlib.md5(stream).hexdigest() == gold["stream_md5"] and hashlib.md5(rec.tobytes()).hexdigest() == gold["frames_md5"]
    plain = dict(RECIPES[name], trace_residual=0)
    assert sg.encode(want_recon=False, **plain)[0] == stream, "trace_residual changed the stream"


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipe_reaches_its_cells(name, sg, oracle_mod):
    """what the yardstick counted on this recipe's trace: nothing the enumeration calls unreachable, and the line of the golden file"""
    cells = _cells(_case(sg, oracle_mod, name)[3])
    print(R.cell_line(name, cells))
    assert R.beyond_reach(cells) == []
    assert R.cell_line(name, cells) in open(COUNTERS_TXT).read().split("\n")


def test_recipes_together_reach_every_cell(sg, oracle_mod):
    """the union of what the recipes reach is the enumeration of what can be reached, but for the cells exempted by name -- at most one in twenty of a
    family, none of qpc, scale, round, scan and matrix; and T is the largest power of two the dequantised coefficients of each class reach"""
    total, max_d = R.Counter(), {}
    for name in RECIPES:
        for p in _case(sg, oracle_mod, name)[3]:
            total.update(p.cells)
            for k, v in p.max_d.items():
                max_d[k] = max(max_d.get(k, 0), v)
    reach = R.reachable_cells()
    missing = sorted((c for c in reach if c not in total), key=repr)
    for family in R.FAMILIES:
        print(family, "enumerated", sum(1 for c in reach if c[0] == family), "reached", sum(1 for c in total if c[0] == family), "exempt", sum(1 for c in R.EXEMPT if c[0] == family))
    print(R.max_line(max_d))
    assert R.beyond_reach(total) == []
    assert sorted(R.EXEMPT, key=repr) == missing, "the cells no recipe reaches are exactly the ones exempted by name"
    assert all(isinstance(why, str) and why and "\n" not in why for why in R.EXEMPT.values())
    for family in R.FAMILIES:
        n = sum(1 for c in reach if c[0] == family)
        ex = sum(1 for c in R.EXEMPT if c[0] == family)
        assert ex * 20 <= n and not (ex and family in R.NO_EXEMPTION), (family, ex, n)
    assert set(max_d) == set(R.T)
    for cls, t in R.T.items():
        assert t & (t - 1) == 0 and t <= max_d[cls] < 2 * t, (cls, t, max_d[cls])
    assert R.max_line(max_d) in open(COUNTERS_TXT).read().split("\n")


def test_enumeration_has_the_shape_the_rules_give():
    reach = R.reachable_cells()

    def n(*head):
        return sum(1 for c in reach if c[:len(head)] == head)
    assert n("qpc") == 108 and n("qpc", "cb") == 54
    assert [n("scale", c) for c in ("luma4", "dc16", "luma8", "cdc", "cac")] == [52, 52, 52, 40, 40]
    # every qP % 6 on both sides of each class's branch: 24 for the 4x4 scaling, 36 for the Intra16x16 DC and the 8x8 scaling; the chroma DC shifts
    # left by qP / 6 and right by 5, so its sides meet at 30
    for cls, pivot in (("luma4", 24), ("dc16", 36), ("luma8", 36), ("cac", 24), ("cdc", 30)):
        for side in (range(0, pivot), range(pivot, R.SCALE_CLASSES[cls])):
            assert {q % 6 for q in side if ("scale", cls, q) in reach} == set(range(6)), (cls, pivot)
    assert n("round") == 8 and ("round", "cdc", "neg") not in reach
    assert n("scan", "frame") == n("scan", "field") == 16 + 64 + 16 + 15 and n("scan", "cb") == n("scan", "cr") == 4
    assert ("scan", "frame", "cac", 0) not in reach and ("scan", "field", "luma8", 63) in reach
    assert n("matrix") == 32
    assert n("cbp", "intra") == n("cbp", "inter") == 48 and n("cbp", "i16") == 6 and ("cbp", "i16", 7, 0) not in reach
    assert n("rows8", "intra") == n("rows8", "inter") == 16
    assert n("chroma") == 7
    # four macroblocks: "others" present with every pair of counts but (2+, 2+); "others" absent only where a 2+ can make up the four
    assert n("group4") == 8 + 5 + 3 and ("group4", 2, 2, 1) not in reach and ("group4", 1, 1, 0) not in reach and ("group4", 2, 2, 0) in reach
    assert n("value", "clip0") == n("value", "clip255") == 9 and n("value", "big") == 5 and n("value") == 33
    assert set(R.FAMILIES) == {c[0] for c in reach}


def test_golden_file_lists_the_recipes():
    assert set(json.load(open(GOLDEN))) == set(RECIPES)
    lines = [ln for ln in open(COUNTERS_TXT).read().split("\n") if ln.startswith("  ") and not ln.startswith("  T:")]
    assert sorted(ln.split()[0] for ln in lines) == sorted(RECIPES)


def test_new_knobs_at_zero_change_nothing(sg):
    """trace_residual and residual_stim at 0 are today's streams, byte for byte (the golden files of the matrices show the same for every recipe there
    is); the trace is a record, not a knob; residual_stim works next to syntax_stim"""
    kw = dict(width=64, height=48, frames=5, idr_period=0, profile_idc=100, cabac=1, transform8x8=1, bframes=1, num_ref_frames=2, pcm_permille=30, seed=5)
    a, rec, _ = sg.encode(**kw)
    assert a == sg.encode(**dict(kw, trace_residual=0, residual_stim=0))[0] and sg.last_residual_trace() == []
    assert a != sg.encode(**dict(kw, residual_stim=1))[0]
    assert a == sg.encode(**dict(kw, residual_stim=2))[0], "only 1 is a stimulus"
    b, rec_b, _ = sg.encode(**dict(kw, trace_residual=1))
    trace = sg.last_residual_trace()
    assert a == b and np.array_equal(rec, rec_b) and len(trace) == 5 and all("rsmbs" in t for t in trace)
    s1 = sg.encode(**dict(kw, syntax_stim=1))[0]
    assert s1 == sg.encode(**dict(kw, syntax_stim=1, trace_residual=1))[0], "the trace is a record under syntax_stim too"
    both, rec_both, _ = sg.encode(**dict(kw, syntax_stim=1, residual_stim=1, trace_residual=1))
    assert both not in (a, s1)
    for t, p in zip(sg.last_residual_trace(), R.reconstruct_stream(sg.last_residual_trace())):
        assert R.first_difference(p, t["planes"]) is None


def test_recipes_cover_what_the_issue_names():
    """the options and sizes the recipes switch on, so that a recipe edited later cannot quietly lose one"""
    main = dict(I_RECIPES, **P_RECIPES, **B_RECIPES, **FIELD_RECIPES, **MONO_RECIPES)
    for name, kw in main.items():
        assert 48 <= kw["width"] <= 96 and 32 <= kw["height"] <= 80 and kw["frames"] <= (5 if kw.get("field_pics") else 8) and kw["trace_residual"] == 1, name
    every = list(RECIPES.values())
    assert sum(1 for k in every if k.get("residual_stim") == 1) * 2 > len(every) and sum(1 for k in every if k.get("residual_stim") and k.get("syntax_stim")) >= 3
    for cabac in (0, 1):
        mine = [k for k in every if k["cabac"] == cabac]
        assert any(k["profile_idc"] in (66, 77) and not k.get("transform8x8") for k in mine) and any(k["profile_idc"] == 100 and k.get("transform8x8") for k in mine)
    assert {k.get("chroma_qp_offset", 0) for k in every} >= {-12, 0, 12}
    assert any(k["profile_idc"] == 100 and k.get("transform8x8") and k.get("chroma_qp_offset", 0) < 12 and not k.get("mono") for k in every), "Cb and Cr differ"
    assert {k.get("scaling_matrix", 0) for k in every} >= {0, 2, 3} and any(k.get("scaling_matrix", 0) >= 2 and k.get("field_pics") == 1 for k in every)
    assert len(I_RECIPES) >= 3 and all(k.get("idr_period", 1) == 1 for k in I_RECIPES.values())
    assert all(not k.get("bframes") and k.get("idr_period", 1) != 1 for k in P_RECIPES.values()) and all(k["bframes"] for k in B_RECIPES.values())
    assert any(k.get("intra_in_p_permille", 0) >= 300 for k in every) and any(k.get("pcm_permille") for k in every)
    assert any(k.get("skip_permille", 0) >= 400 for k in every) and any(k.get("slices") == 3 for k in every)
    assert {k["field_pics"] for k in FIELD_RECIPES.values()} >= {1, 3}
    assert any(k["field_pics"] == 1 and not k["cabac"] for k in FIELD_RECIPES.values())
    assert any(k["cabac"] and decoder_cfg(k) for k in FIELD_RECIPES.values())
    assert any(k.get("mono") == 1 and k.get("transform8x8") for k in every)
    assert any(k.get("contrast") == 1 and k["qp"] == 4 for k in every) and any(k.get("contrast") == 1 and k["qp"] == 51 for k in every)
    for group in (I_RECIPES, P_RECIPES, B_RECIPES, FIELD_RECIPES):
        assert any(k.get("deblock_idc") == 1 for k in group.values())
    assert sorted((k["width"], k["height"]) for k in GEOMETRY.values()) == sorted([(16, 16), (176, 16), (16, 144), (32, 32)])
    assert all(k["frames"] == 3 for k in GEOMETRY.values())


def _all_equal(trace):
    return all(R.first_difference(p, t["planes"]) is None for t, p in zip(trace, R.reconstruct_stream(trace)))


def test_a_wrong_rule_in_the_yardstick_is_noticed(sg, oracle_mod, monkeypatch):
    """the comparison has teeth: each misreading of 8.5, patched into the yardstick, is found on a named recipe"""
    base = _case(sg, oracle_mod, "i_cavlc_base")[2]
    field = _case(sg, oracle_mod, "field_cavlc_high8_sm2")[2]
    high = _case(sg, oracle_mod, "p_cavlc_high8")[2]
    assert _all_equal(base) and _all_equal(field) and _all_equal(high)
    monkeypatch.setattr(R, "_round_term", lambda shift: 0)                     # the rounding term dropped below the shift branch
    assert not _all_equal(base)
    monkeypatch.undo()
    scan_for = R._scan_for
    monkeypatch.setattr(R, "_scan_for", lambda n, fld: scan_for(n, not fld))   # field scan and zig-zag swapped
    assert not _all_equal(field) and not _all_equal(base)
    monkeypatch.undo()
    qpc = R._qpc
    monkeypatch.setattr(R, "_qpc", lambda plane, qp, offsets: qpc(1, qp, offsets))   # Cr given Cb's QPc
    assert not _all_equal(high)
    monkeypatch.undo()
    monkeypatch.setattr(R, "_shr", lambda x, n: np.where(x < 0, -((-x) >> n), x >> n))   # ">> 1" as a division towards zero
    assert not _all_equal(base) and not _all_equal(high)
    monkeypatch.undo()
    monkeypatch.setattr(R, "_PIVOT_DC16", R._PIVOT_4x4)                        # the Intra16x16 DC scaled with the 4x4 branch point
    assert not _all_equal(base)
    monkeypatch.undo()
    assert _all_equal(base)


# ---- GPU ----
GENERAL, FMO, CABAC, MAIN = 0, 1, 2, 3   # h264mi_internal_entropy_kernel_choice4


def _decode(H, items, x_wgs=None, side=False):
    """items: [(kw, stream)] decoded as ONE batch; per stream (frames uncropped -- every size here is a multiple of 16 --, and with `side` the qp and nz
    planes of its frames as numpy [frame, plane, gh, gw])"""
    from test_entropy_main_gpu import _nslices
    from test_gpu_parity import _x_wgs
    cfg = {}
    for kw, _ in items:
        cfg.update(decoder_cfg(kw))
    with _x_wgs(x_wgs):
        dec = H.Decoder(max_streams=len(items), max_width=max(kw["width"] for kw, _ in items), max_height=max(kw["height"] for kw, _ in items),
                        max_frames_per_batch=max(pictures_of(kw) for kw, _ in items), max_slices_per_frame=max(_nslices(kw) for kw, _ in items),
                        max_bitstream_bytes=sum(len(s) for _, s in items) * 2 + (1 << 20), **cfg)
        try:
            dec.decode([s for _, s in items])
            out = []
            for i, (kw, _) in enumerate(items):
                frames = dec.read_frames(i, crop=True, size=kw["width"] * kw["height"] * 3 // 2)
                planes = np.stack([v.cpu().numpy() for v in dec.side_info(stream=i, planes=("qp", "nz"))]) if side and not kw.get("field_pics") else None
                out.append((frames, planes))
            return out
        finally:
            dec.close()


def _first_wrong_macroblock(kw, frames, rec, trace, pics):
    """(frame, macroblock address in its picture, the yardstick's class words of its blocks) of the first sample that differs"""
    W, Hc = kw["width"], kw["height"]
    f = next(i for i in range(len(rec)) if not np.array_equal(frames[i], rec[i]))
    for plane, (got, want) in enumerate(zip(_frame_planes(frames[f], W, Hc), _frame_planes(rec[f], W, Hc))):
        bad = np.argwhere(got != want)
        if len(bad):
            y, x = (int(v) for v in bad[0])
            n = 16 if plane == 0 else 8
            for t, p in zip(trace, pics):
                if t["frame"] == f and (t["field"] == 0 or t["field"] - 1 == (y & 1)):
                    addr = ((y >> 1 if t["field"] else y) // n) * p.wmb + x // n
                    return f, plane, addr, R.macroblock_words(p, addr)
    return f, None, None, None


def _check(name, got, case, what):
    kw = RECIPES[name]
    frames, side = got
    stream, rec, trace, pics, ref = case
    assert frames.shape == rec.shape, (name, what)
    if not np.array_equal(frames, rec):
        raise AssertionError(("GPU != generator reconstruction: (frame, plane, macroblock, the yardstick's class words of its blocks)", name, what,
                              _first_wrong_macroblock(kw, frames, rec, trace, pics)))
    assert np.array_equal(frames, ref), ("GPU != oracle", name, what)
    assert hashlib.md5(frames.tobytes()).hexdigest() == json.load(open(GOLDEN))[name]["frames_md5"], (name, what)
    if side is not None:
        assert side.shape[0] == len(pics), (name, what)
        for t, p in zip(trace, pics):
            f = t["frame"]
            want_qp = np.repeat(np.repeat(np.where(t["rsmbs"]["kind"] == R.RS_PCM, 0, p.qp), 4, axis=0), 4, axis=1)
            for i, (plane, want) in enumerate((("qp", want_qp), ("nz", p.nz))):
                assert side[f][i].shape == want.shape, (name, what, plane)
                bad = np.argwhere(side[f][i] != want)
                assert not len(bad), ("GPU != yardstick", name, what, "frame", f, plane, "first (block row, block column)", bad[0].tolist(),
                                      int(side[f][i][tuple(bad[0])]), int(want[tuple(bad[0])]))


_P_MAIN = sorted(n for n, kw in RECIPES.items() if R.main_eligible(kw))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RECIPES))
def test_gpu_equals_generator_oracle_and_yardstick(name, H, sg, oracle_mod):
    """the banded kernels of K3 / K5, and a picture inside one workgroup; B recipes on k_entropy_b, field recipes on the field kernel"""
    kw, case = RECIPES[name], _case(sg, oracle_mod, name)
    for x_wgs in (None, 0):
        _check(name, _decode(H, [(kw, case[0])], x_wgs, side=True)[0], case, ("alone", x_wgs))


@pytest.mark.gpu
@pytest.mark.parametrize("name", _P_MAIN)
def test_gpu_p_cabac_residual_on_three_routes(name, H, sg, oracle_mod):
    """alone on k_entropy_m, next to an 8x8-transform stream on k_entropy_c, next to a CAVLC stream on k_entropy: the inverse scans are in each build"""
    from test_entropy_main_gpu import _route
    kw, case = RECIPES[name], _case(sg, oracle_mod, name)
    t8_name, cav_name = "i_cabac_high8_cqo_m12_pcm", "i_cavlc_base"
    t8_kw, cav_kw = RECIPES[t8_name], RECIPES[cav_name]
    assert t8_kw["cabac"] == 1 and t8_kw["transform8x8"] == 1 and cav_kw["cabac"] == 0
    assert _route(H, [kw]) == MAIN and _route(H, [kw, t8_kw]) == CABAC and _route(H, [kw, cav_kw]) == GENERAL
    t8, cav = _case(sg, oracle_mod, t8_name), _case(sg, oracle_mod, cav_name)
    _check(name, _decode(H, [(kw, case[0])])[0], case, "alone: k_entropy_m")
    both = _decode(H, [(kw, case[0]), (t8_kw, t8[0])])
    _check(name, both[0], case, "next to an 8x8-transform stream: k_entropy_c")
    _check(t8_name, both[1], t8, "the 8x8-transform stream of that batch")
    both = _decode(H, [(kw, case[0]), (cav_kw, cav[0])])
    _check(name, both[0], case, "next to a CAVLC stream: k_entropy")
    _check(cav_name, both[1], cav, "the CAVLC stream of that batch")


@pytest.mark.gpu
def test_gpu_batch_of_four_recipes(H, sg, oracle_mod):
    """flat 4x4 P, coded-matrix 8x8 B, a field recipe and a monochrome one in ONE batch: scaling sets, QPc and the coefficient pool are per-picture state
    of launches the four share"""
    names = ["p_cabac_main_intra", "b_cabac_high8_sm2", "field_cavlc_high8_sm2", "mono_cabac_high8"]
    kws = [RECIPES[n] for n in names]
    assert not kws[0].get("scaling_matrix") and not kws[0].get("transform8x8") and kws[1]["scaling_matrix"] == 2 and kws[1]["transform8x8"] and kws[1]["bframes"]
    assert kws[2]["field_pics"] == 1 and kws[3]["mono"] == 1
    cases = [_case(sg, oracle_mod, n) for n in names]
    for x_wgs in (None, 0):
        got = _decode(H, [(kw, c[0]) for kw, c in zip(kws, cases)], x_wgs, side=True)
        for n, g, c in zip(names, got, cases):
            _check(n, g, c, ("batch of four", x_wgs))
