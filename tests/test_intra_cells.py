"""Intra prediction (8.3) cell by cell on whole pictures (recipes: tests/intrautil.py).  A cell is (Intra4x4 / Intra8x8 / Intra16x16 / chroma, prediction
mode, the combination of left / top / top-left / top-right neighbours the block sees).

On the CPU: the generator's prediction samples against the numpy yardstick applied to the generator's own trace (the picture before the deblocking
filter, the macroblock kinds, modes and slices) -- a fourth writing of 8.3 and of the availability rules, independent of generator, oracle and product
--, the oracle against the generator, the golden MD5s, and the generator's counters, which must show that each recipe reaches the cells it claims (and
which the yardstick counts once more from its class words: the two counts must be equal).  The set of reachable cells is enumerated by the yardstick;
the recipes together must ask for exactly that set.

On the GPU: every recipe through k_intra_x and through k_intra, bit for bit against generator, oracle and golden MD5; the geometry recipes also with so
few workgroups that a band of k_intra_x holds many rows; four unlike recipes in one batch.  There is no tolerance anywhere in this file."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import deblockutil as D
import intrautil as I
from intrautil import CONTENT, GEOMETRY, RECIPES, pictures_of
from rangeutil import decoder_cfg

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "intra_md5.json")
COUNTERS_TXT = os.path.join(os.path.dirname(__file__), "golden", "intra_counters.txt")
_cache = {}


def _case(sg, oracle_mod, name):
    """(stream, generator reconstruction, counters, trace, oracle frames) of a recipe: made once, not modified"""
    if name not in _cache:
        stream, rec, _ = sg.encode(trace_intra=1, **RECIPES[name])
        ranges, trace = sg.last_ranges(), sg.last_intra_trace()
        ref, _ = oracle_mod.decode(stream, crop=False)
        for a in (rec, ref):
            a.setflags(write=False)
        _cache[name] = (stream, rec, ranges, trace, ref)
    return _cache[name]


def _frame_planes(frame, w, h):
    return frame[:w * h].reshape(h, w), frame[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), frame[w * h * 5 // 4:].reshape(h // 2, w // 2)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_yardstick_equals_generator(name, sg, oracle_mod):
    """the independent pin: 8.3 in numpy on the picture before sg_deblock gives the generator's prediction sample for every intra-predicted sample, and
    counts what it counted; the picture, deblocked by the yardstick of 8.7, is the reconstruction's"""
    kw = RECIPES[name]
    stream, rec, ranges, trace, _ = _case(sg, oracle_mod, name)
    if kw.get("field_pics") == 3:  # picture-adaptive: frame pictures and field pictures in one stream
        assert kw["frames"] < len(trace) < pictures_of(kw) and {t["field"] for t in trace} == {0, 1, 2}
    else:
        assert len(trace) == pictures_of(kw)
    W, H = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
    counters = I.new_counters()
    for i, t in enumerate(trace):
        assert t["mono"] == kw.get("mono", 0) and t["constrained_intra"] == kw.get("constrained_intra", 0), i
        if kw.get("field_pics", 0) in (1, 2):
            assert t["field"] != 0, i
        pred, mask, c = I.predict_picture(t)
        I.merge(counters, c)
        for plane in range(1 if t["mono"] else 3):
            kinds = np.repeat(np.repeat(t["ipmbs"]["kind"], mask[plane].shape[0] // t["ipmbs"].shape[0], axis=0), mask[plane].shape[1] // t["ipmbs"].shape[1], axis=1)
            assert np.array_equal(mask[plane], (kinds >= I.KIND_I4) & (kinds <= I.KIND_I16)), (name, i, plane)
            bad = mask[plane] & (pred[plane] != t["pred"][plane])
            assert not bad.any(), ("yardstick != generator", name, "picture", i, "plane", plane, np.argwhere(bad)[:4].tolist())
            assert not (~mask[plane] & ((t["pred"][plane] != 0) | (t["res"][plane] != 0))).any(), ("the trace has samples outside intra macroblocks", name, i, plane)
        # ... and those are the pictures the reconstruction is made of: deblocked (the yardstick of 8.7), in the rows of the field's parity
        out = D.deblock_picture(t["planes"], t["mbs"], t["field"] != 0, t["mono"])
        rows = slice(None) if t["field"] == 0 else slice(t["field"] - 1, None, 2)
        for plane, (got, whole) in enumerate(zip(out, _frame_planes(rec[t["frame"]], W, H))):
            if not (t["mono"] and plane):
                assert np.array_equal(got, t["after"][plane]) and np.array_equal(whole[rows], got), ("trace, deblocked, != reconstruction", name, i, plane)
    differ = {k: (ranges[k], counters[k]) for k in I.COUNTERS if ranges[k] != counters[k]}
    assert not differ, ("generator's counters != the yardstick's (generator, yardstick)", differ)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_oracle_equals_generator(name, sg, oracle_mod):
    stream, rec, _, _, ref = _case(sg, oracle_mod, name)
    assert ref.shape == rec.shape and np.array_equal(ref, rec), "oracle != generator reconstruction"
    gold = json.load(open(GOLDEN))[name]
    assert hashlib.md5(stream).hexdigest() == gold["stream_md5"] and hashlib.md5(rec.tobytes()).hexdigest() == gold["frames_md5"]
    assert sg.encode(want_recon=False, **RECIPES[name])[0] == stream, "trace_intra changed the stream"


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipe_reaches_its_cells(name, sg, oracle_mod):
    """What the generator counted in encode_intra on the modes it chose for this recipe: the cells and counters the recipe claims, and the line of the golden file."""
    ranges = _case(sg, oracle_mod, name)[2]
    print(I.counter_line(name, ranges))
    assert I.unmet(name, ranges) == []
    assert not I.cells_of(ranges) - I.reachable_cells(), "a cell the enumeration calls unreachable"
    assert I.counter_line(name, ranges) in open(COUNTERS_TXT).read().split("\n")


def test_every_cell_is_required_by_a_recipe():
    """the union of what the recipes ask for is the yardstick's enumeration of what can be reached -- no cell more, no cell less"""
    cells = I.reachable_cells()
    per_slot = {s: sum(1 for c in cells if c[0] == s) for s in I.SLOTS}
    allowed = {s: sum(1 for m in range(I.NMODES[s]) for cb in range(16) if I.mode_allowed(s, m, cb)) for s in I.SLOTS}
    print("reachable cells", per_slot, "of the mode-allowed", allowed)
    # what the enumeration must show whatever its size: every mode of every kind in some cell, and Intra16x16 / chroma see all 16 neighbourhoods (DC is always allowed)
    assert {(s, m) for s, m, _ in cells} == {(s, m) for s in I.SLOTS for m in range(I.NMODES[s])}
    assert all({cb for s, m, cb in cells if s == slot and m == dc} == set(range(16)) for slot, dc in (("16", 2), ("c", 0)))
    # a block's top-right and top differ only where the block is the last of the macroblock's top row (left is there then), or later in the scan than its top-right neighbour
    assert all(per_slot[s] < allowed[s] for s in ("4", "8")) and all(per_slot[s] == allowed[s] for s in ("16", "c"))
    assert I.required_somewhere() == [] and I.required_beyond_reach() == []


def test_golden_file_lists_the_recipes():
    assert set(json.load(open(GOLDEN))) == set(RECIPES) == set(I.NEED)
    lines = [ln for ln in open(COUNTERS_TXT).read().split("\n") if ln.startswith("  ")]
    assert sorted(ln.split()[0] for ln in lines) == sorted(RECIPES)


def test_new_knobs_at_zero_change_nothing(sg):
    """intra_stim and trace_intra at 0 are today's streams, byte for byte (the golden files of the matrices show the same for every recipe there is); the
    trace is a record, not a knob"""
    kw = dict(width=64, height=48, frames=4, idr_period=0, profile_idc=100, cabac=1, transform8x8=1, slices=2, intra_in_p_permille=300, seed=5)
    a, rec, _ = sg.encode(**kw)
    assert a == sg.encode(**dict(kw, intra_stim=0, trace_intra=0, direct_4x4=0, trace_motion=0, motion_stim=0))[0] and sg.last_intra_trace() == []
    assert sg.last_motion_trace() == []
    m, rec_m, _ = sg.encode(**dict(kw, trace_motion=1))
    assert a == m and np.array_equal(rec, rec_m) and len(sg.last_motion_trace()) == 4 and sg.last_intra_trace() == []
    b, rec_b, _ = sg.encode(**dict(kw, trace_intra=1))
    assert a == b and np.array_equal(rec, rec_b) and len(sg.last_intra_trace()) == 4 and "pred" in sg.last_intra_trace()[0]
    sg.encode(**dict(kw, trace_deblock=1))
    assert len(sg.last_intra_trace()) == 4 and "pred" not in sg.last_intra_trace()[0], "trace_deblock alone keeps no prediction samples"
    assert a != sg.encode(**dict(kw, intra_stim=1))[0]
    assert a == sg.encode(**dict(kw, intra_stim=2))[0], "only 1 is a stimulus"


def test_recipes_cover_what_the_issue_names():
    """the options and sizes the recipes switch on, so that a recipe edited later cannot quietly lose one"""
    ks = list(CONTENT.values())
    for kw in ks:
        assert pictures_of(kw) <= 24 and 64 <= kw["width"] <= 96 and 48 <= kw["height"] <= 80 and kw["intra_stim"] == 1, kw
    con = [k for k in ks if k.get("constrained_intra") and 450 <= k.get("intra_in_p_permille", 0) <= 550 and not k.get("transform8x8")]
    assert any(k["cabac"] for k in con) and any(not k["cabac"] for k in con)
    free = [k for k in ks if not k.get("constrained_intra") and k.get("pcm_permille", 0) > 0 and k.get("intra_in_p_permille", 0) >= 400]
    assert any(k["cabac"] for k in free) and any(not k["cabac"] for k in free)
    assert any(k["profile_idc"] == 100 and k.get("transform8x8") and k.get("constrained_intra") for k in ks)
    assert any(k.get("bframes") and k.get("intra_in_p_permille", 0) > 0 for k in ks)
    assert any(k.get("field_pics") in (1, 2) and not k["cabac"] for k in ks)
    assert any(k.get("field_pics") == 3 and k["cabac"] and decoder_cfg(k) for k in ks)
    assert any(k.get("mono") for k in ks)
    assert any(k.get("slice_groups") == 2 and k.get("fmo_type") == 1 for k in ks)
    assert any(k.get("slice_groups", 0) > 1 and k.get("fmo_type") == 6 and k.get("aso") for k in ks)
    assert any(k.get("slices") == 3 and k["width"] == 80 and not k.get("slice_groups") for k in ks)
    assert sum(1 for k in ks if k.get("contrast")) >= 1
    geo = sorted((kw["width"], kw["height"], kw["idr_period"] == 1) for kw in GEOMETRY.values())
    assert geo == sorted([(16, 16, True), (16, 16, False), (272, 16, True), (272, 16, False), (16, 272, True), (16, 272, False), (1040, 80, True), (1040, 80, False),
                          (1040, 80, False)])
    assert all(not kw.get("constrained_intra") for kw in GEOMETRY.values())
    assert sorted(kw["intra_in_p_permille"] for kw in GEOMETRY.values() if kw["width"] == 1040 and kw["idr_period"] == 0) == [150, 500]


def test_content_recipes_reach_what_their_family_is_for(sg, oracle_mod):
    """by family, in words of neighbourhoods (the masks of intrautil.NEED say the same cell by cell)"""
    def r(name):
        return _case(sg, oracle_mod, name)[2]
    # all 16 neighbourhoods of a macroblock, out of inter neighbours that may not be predicted from
    for name in ("constrained_p_cabac", "constrained_p_cavlc"):
        assert r(name)["ip_avc_m0"] == 0xFFFF and r(name)["ip_from_inter"] == 0 and r(name)["ip_from_pcm"] == 0
    # samples K4 wrote and I_PCM samples, from all four directions
    for name in ("k4_samples_pcm_cabac", "k4_samples_pcm_cavlc_8x8"):
        assert r(name)["ip_from_inter"] == 15 and r(name)["ip_from_pcm"] == 15
    # the checkerboard: above left and above right without above and left (combination 12), chroma DC and Intra16x16 DC
    assert r("fmo_checkerboard_cavlc")["ip_avc_m0"] >> 12 & 1 and r("fmo_checkerboard_cavlc")["ip_av16_m2"] >> 12 & 1
    # slices that start in the middle of a row: above right without above (8 or 9), above and left without above left (3 or 11)
    for name in ("slices3_midrow_cabac", "slices3_midrow_cavlc_8x8"):
        m = r(name)["ip_avc_m0"]
        assert m & (1 << 8 | 1 << 9) and m & (1 << 3 | 1 << 11), (name, hex(m))
    assert r("slices3_midrow_cavlc_8x8")["ip_f8_top_no_tl"] > 0 and r("slices3_midrow_cavlc_8x8")["ip_f8_left_no_tl"] > 0
    for name in ("contrast_cabac_8x8", "contrast_cavlc"):
        assert all(r(name)[k] > 0 for k in ("ip_planec_lo", "ip_planec_hi", "ip_rec_luma_at0", "ip_rec_luma_at255", "ip_rec_chroma_at0", "ip_rec_chroma_at255")), name
    assert r("contrast_cavlc")["ip_plane16_lo"] > 0 and r("contrast_cavlc")["ip_plane16_hi"] > 0
    assert r("mono_cabac_8x8")["ip_avc_m0"] == 0, "no chroma cell in a monochrome stream"


# ---- the schedules of K3 (k_recon.hip), as far as the CPU can see them: which pictures take which path ----
def _intra_plan(H, n_pics, hmb, max_wgs, p_only, band=1):
    f = H.load_hooks().h264mi_internal_intra_plan
    I32 = ctypes.c_int32
    f.restype, f.argtypes = I32, [I32] * 5 + [ctypes.POINTER(I32)] * 4
    v = [I32() for _ in range(4)]
    assert f(n_pics, hmb, max_wgs, int(p_only), band, *[ctypes.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)  # bands, wavefronts, wavefronts per row, first row of `band`


X_WGS_FEW = 2  # the workgroups of the geometry recipes' extra run: two bands per picture


def test_geometry_recipes_reach_the_schedules(H, sg, oracle_mod):
    """from the trace and from the launch plan (a single stream: every picture is a launch of its own, reconstruction wave by wave)"""
    sides = set()
    for name, kw in sorted(GEOMETRY.items()):
        trace = _case(sg, oracle_mod, name)[3]
        wmb, hmb = (kw["width"] + 15) // 16, (kw["height"] + 15) // 16
        p_variant = kw["idr_period"] == 0
        for i, t in enumerate(trace):
            intra = t["ipmbs"]["kind"] != I.KIND_INTER       # what K3 owns: intra-predicted and I_PCM macroblocks
            assert wmb * hmb == 1 or intra.all() == (i == 0 or not p_variant), (name, i)
            if not intra.all():
                if wmb == 65:
                    sides.add(bool(intra.sum() * 4 < wmb * hmb))   # k_intra: sparse / dense dealing
        if p_variant:  # intra macroblocks among inter ones (a picture of one macroblock: a P picture that is an intra macroblock, and one that is not)
            kinds = [t["ipmbs"]["kind"] for t in trace[1:]]
            assert any(((k >= I.KIND_I4) & (k <= I.KIND_I16)).any() for k in kinds) and any((k == I.KIND_INTER).any() for k in kinds), name
            assert wmb * hmb == 1 or any(((k >= I.KIND_I4) & (k <= I.KIND_I16)).any() and (k == I.KIND_INTER).any() for k in kinds), name
        if hmb == 17:  # more rows than k_intra has wavefronts: wavefront 0 takes a second row; k_intra_x: several bands, with few workgroups bands of several rows
            bands, waves, wpr, row0 = _intra_plan(H, 1, hmb, 256, False)
            assert waves < hmb and bands > 2 and 0 < row0
            bands, waves, wpr, row0 = _intra_plan(H, 1, hmb, X_WGS_FEW, False)
            assert bands == 2 and row0 >= 8
        if wmb != 65:
            continue
        # 65 columns (0 .. 64): what macroblock columns 63 and 64 wait for in the row above straddles the chunks of 64 columns (AboveSpan).  Intra macroblocks
        # at columns 62, 63 and 64 of a row and at 63 or 64 in the row below, in the first row of the second band (another workgroup's flags) and in a row inside
        # a band (the LDS masks)
        for p_only in ((False, True) if p_variant else (False,)):
            pics = [t for i, t in enumerate(trace) if (i > 0) == p_only]
            for max_wgs in (256, X_WGS_FEW):
                bands, waves, wpr, row0 = _intra_plan(H, 1, hmb, max_wgs, p_only)
                assert bands == 2 and 0 < row0 < hmb
                if p_only:
                    assert wpr > 1, "P pictures: several wavefronts per row"
                inside = [r for r in range(1, hmb) if r != row0]
                ks = [t["ipmbs"]["kind"] != I.KIND_INTER for t in pics]
                if kw.get("intra_in_p_permille") == 150 and p_only:
                    # the sparse pictures (fifteen macroblocks in a hundred are intra ones): an intra macroblock at column 63 or 64 below one of the first chunk's
                    # last columns, and one below column 64, the second chunk's only one -- both masks of AboveSpan are waited on, if not by one macroblock
                    for cols, what in (((62, 63), "the first chunk"), ((64,), "the second chunk")):
                        assert any(k[r, c] and k[r - 1, x] for k in ks for r in range(1, hmb) for c in (63, 64) for x in cols if abs(x - c) <= 1), (name, what)
                    continue
                for rows, what in (([row0], "the first row of the second band"), (inside, "a row inside a band")):
                    assert any((k[r, 63] or k[r, 64]) and k[r - 1, 62] and k[r - 1, 63] and k[r - 1, 64] for k in ks for r in rows), (name, what, "p_only", p_only)
    assert sides == {True, False}, "P pictures on both sides of n_intra * 4 < wmb * hmb"


# ---- GPU ----
def _decode(H, kw, stream, x_wgs):
    from test_gpu_parity import _decode_gpu, _nslices
    out, info = _decode_gpu(H, [stream], kw["width"], kw["height"], pictures_of(kw), _nslices(kw), x_wgs=x_wgs, **decoder_cfg(kw))
    assert info.n_frames == kw["frames"]
    return out[0]


def _check(name, out, case, what):
    stream, rec, _, _, ref = case
    assert out.shape == rec.shape, (name, what)
    assert np.array_equal(out, rec), ("GPU != generator reconstruction", name, what, [i for i in range(len(rec)) if not np.array_equal(out[i], rec[i])])
    assert np.array_equal(out, ref), ("GPU != oracle", name, what)
    assert hashlib.md5(out.tobytes()).hexdigest() == json.load(open(GOLDEN))[name]["frames_md5"], (name, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RECIPES))
def test_gpu_equals_generator_and_oracle(name, H, sg, oracle_mod):
    kw, case = RECIPES[name], _case(sg, oracle_mod, name)
    for x_wgs in (None, 0):  # k_intra_x (a picture spread over workgroups), k_intra (a picture inside one workgroup)
        _check(name, _decode(H, kw, case[0], x_wgs), case, "x_wgs %s" % x_wgs)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_gpu_geometries_with_few_workgroups(name, H, sg, oracle_mod):
    """k_intra_x with two bands per picture: a band of 17 rows holds eight or nine of them"""
    kw, case = RECIPES[name], _case(sg, oracle_mod, name)
    _check(name, _decode(H, kw, case[0], X_WGS_FEW), case, "x_wgs %d" % X_WGS_FEW)


@pytest.mark.gpu
def test_gpu_batch_of_four_recipes(H, sg, oracle_mod):
    """Constrained intra prediction, the checkerboard of two slice groups, field pictures and the 65-column P stream in ONE batch of one decoder."""
    from test_gpu_parity import _decode_gpu, _nslices
    names = ["constrained_p_cabac", "fmo_checkerboard_cavlc", "field_cavlc", "geo_1040x80_p500"]
    cases = [_case(sg, oracle_mod, n) for n in names]
    kws = [RECIPES[n] for n in names]
    for x_wgs in (None, 0):
        out, info = _decode_gpu(H, [c[0] for c in cases], max(k["width"] for k in kws), max(k["height"] for k in kws), max(pictures_of(k) for k in kws),
                                max(_nslices(k) for k in kws), x_wgs=x_wgs)
        for i, n in enumerate(names):
            W, Hc = (kws[i]["width"] + 15) & ~15, (kws[i]["height"] + 15) & ~15
            assert out[i].shape[0] == kws[i]["frames"], n
            assert np.array_equal(out[i][:, :W * Hc * 3 // 2], cases[i][1]), (n, x_wgs)
