"""Deblocking (8.7) branch by branch on whole pictures (recipes: tests/deblockutil.py).

On the CPU: the generator's deblocked pictures against the numpy yardstick applied to the generator's own trace (planes before the filter + the
macroblock table) -- a fourth writing of 8.7, independent of generator, oracle and product --, the oracle against the generator, the golden MD5s,
and the generator's counters, which must show that each recipe takes the branches it claims to take (and which the yardstick counts once more
from its class words: the two counts must be equal).

On the GPU: every recipe through k_deblock_x and through k_deblock, bit for bit against generator and oracle, with k_dbprep_ip / k_dbprep checked
against k_dbprep by the hook; the geometry recipes with 8, 2 and 1 wavefronts per picture in k_deblock (a wavefront's second and third round over a
picture, the two-buffer plan of the last ring); four unlike recipes in one batch.  There is no tolerance anywhere in this file."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import deblockutil as D
from deblockutil import CONTENT, GEOMETRY, RECIPES, pictures_of

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "deblock_md5.json")
_cache = {}


def _case(sg, oracle_mod, name):
    """(stream, generator reconstruction, counters, trace, oracle frames) of a recipe: made once, not modified"""
    if name not in _cache:
        stream, rec, _ = sg.encode(trace_deblock=1, **RECIPES[name])
        ranges, trace = sg.last_ranges(), sg.last_deblock_trace()
        ref, _ = oracle_mod.decode(stream, crop=False)
        for a in (rec, ref):
            a.setflags(write=False)
        _cache[name] = (stream, rec, ranges, trace, ref)
    return _cache[name]


def _frame_planes(frame, w, h):
    return frame[:w * h].reshape(h, w), frame[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), frame[w * h * 5 // 4:].reshape(h // 2, w // 2)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_yardstick_equals_generator(name, sg, oracle_mod):
    """the independent pin: 8.7 in numpy on the planes before sg_deblock and the macroblock table gives the generator's pictures, and counts what it counted"""
    kw = RECIPES[name]
    stream, rec, ranges, trace, _ = _case(sg, oracle_mod, name)
    assert len(trace) == pictures_of(kw)
    W, H = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
    counters = D.new_counters()
    for i, t in enumerate(trace):
        assert t["mono"] == kw.get("mono", 0) and (t["field"] != 0) == bool(kw.get("field_pics")), i
        out = D.deblock_picture(t["planes"], t["mbs"], t["field"] != 0, t["mono"], counters)
        for plane, (got, want) in enumerate(zip(out, t["after"])):
            assert np.array_equal(got, want), ("yardstick != generator", name, "picture", i, "plane", plane, np.argwhere(got != want)[:4].tolist())
        # ... and those are the pictures the reconstruction is made of (a field: the rows of its parity)
        rows = slice(None) if t["field"] == 0 else slice(t["field"] - 1, None, 2)
        for plane, (want, whole) in enumerate(zip(t["after"], _frame_planes(rec[t["frame"]], W, H))):
            if not (t["mono"] and plane):
                assert np.array_equal(whole[rows], want), ("trace != reconstruction", name, i, plane)
    differ = {k: (ranges[k], counters[k]) for k in D.COUNTERS if ranges[k] != counters[k]}
    assert not differ, ("generator's counters != the yardstick's (generator, yardstick)", differ)


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_oracle_equals_generator(name, sg, oracle_mod):
    stream, rec, _, _, ref = _case(sg, oracle_mod, name)
    assert ref.shape == rec.shape and np.array_equal(ref, rec), "oracle != generator reconstruction"
    gold = json.load(open(GOLDEN))[name]
    assert hashlib.md5(stream).hexdigest() == gold["stream_md5"] and hashlib.md5(rec.tobytes()).hexdigest() == gold["frames_md5"]
    assert sg.encode(want_recon=False, **RECIPES[name])[0] == stream, "trace_deblock changed the stream"


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipe_reaches_its_branches(name, sg, oracle_mod):
    """What the generator counted in sg_deblock on the final reconstruction of this recipe."""
    ranges = _case(sg, oracle_mod, name)[2]
    print(name, {k[3:]: v for k, v in ranges.items() if k.startswith("db_") and v and abs(v) != 1 << 20})
    assert D.unmet(name, ranges) == []


def test_every_counter_is_required_by_a_recipe():
    assert D.required_somewhere() == []


def test_golden_file_lists_the_recipes():
    assert set(json.load(open(GOLDEN))) == set(RECIPES)


def test_recipes_cover_what_the_issue_names():
    """the options and sizes the recipes switch on, so that a recipe edited later cannot quietly lose one"""
    ks = [kw for kw, _ in CONTENT.values()]
    for kw in ks:
        assert 4 <= kw["frames"] <= 7 and 64 <= kw["width"] <= 96 and 48 <= kw["height"] <= 80, kw
    assert any(k["cabac"] for k in ks) and any(not k["cabac"] for k in ks)
    assert any(k.get("qp_jitter") and k.get("pcm_permille") for k in ks)
    assert any(k.get("alpha_off_div2") == -6 for k in ks) and any(k.get("alpha_off_div2") == 6 for k in ks)
    assert any(k.get("chroma_qp_offset") == -12 and k["profile_idc"] == 100 for k in ks) and any(k.get("chroma_qp_offset") == 12 for k in ks)
    assert any(k.get("transform8x8") for k in ks) and any(k.get("mono") for k in ks)
    assert any(k.get("slices") == 3 and k.get("dbf_per_slice") for k in ks)
    assert any(k.get("bframes") and k.get("direct_temporal") for k in ks) and any(k.get("bframes") and not k.get("direct_temporal") for k in ks)
    assert any(k.get("bframes") and k.get("num_ref_frames", 1) >= 3 and k.get("wp_range") == 2 for k in ks)
    assert any(k.get("field_pics") and not k["cabac"] and not k.get("bframes") for k in ks) and any(k.get("field_pics") and k.get("bframes") for k in ks)
    assert sorted((kw["width"], kw["height"]) for kw, _ in GEOMETRY.values()) == [(16, 16), (16, 272), (80, 144), (80, 272), (272, 16), (1040, 32)]


# ---- GPU ----
def _decode(H, kw, stream, x_wgs, k5_waves=None):
    """the stream decoded as one batch: (frames, launches k_dbprep_ip, launches k_dbprep, bytes of the DbPrm records / intra mask that differ from k_dbprep's)"""
    from test_gpu_parity import _x_wgs
    W, Hc = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
    with _x_wgs(x_wgs):
        dec = H.Decoder(max_streams=1, max_width=W, max_height=Hc, max_frames_per_batch=pictures_of(kw), max_slices_per_frame=max(1, kw.get("slices", 1)),
                        max_bitstream_bytes=len(stream) * 2 + (1 << 20))
    try:
        hooks = H.load_hooks()
        if k5_waves is not None:
            assert hooks.h264mi_internal_set_k5_waves(dec._h, k5_waves) == 0
        info = dec.decode([stream])
        assert info.n_frames == kw["frames"]
        out = dec.read_frames(0, crop=False, size=W * Hc * 3 // 2)
        ip, gen, bad = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1)
        assert hooks.h264mi_internal_dbprep_check(dec._h, ctypes.byref(ip), ctypes.byref(gen), ctypes.byref(bad)) == 0
        return out, ip.value, gen.value, bad.value
    finally:
        dec.close()


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
    for x_wgs in (None, 0):  # k_deblock_x (a picture spread over workgroups), k_deblock (a picture inside one workgroup)
        out, ip, gen, bad = _decode(H, kw, case[0], x_wgs)
        print("%s, x_wgs %s: launches k_dbprep_ip %d, k_dbprep %d, mismatching bytes %d" % (name, x_wgs, ip, gen, bad))
        _check(name, out, case, "x_wgs %s" % x_wgs)
        assert bad == 0, "%d bytes of the DbPrm records / intra mask differ from k_dbprep's (x_wgs %s)" % (bad, x_wgs)
        if kw.get("bframes"):
            assert gen > 0, "a batch with B pictures launches k_dbprep"
        else:
            assert ip > 0 and gen == 0, "a batch of I / P pictures runs on k_dbprep_ip alone"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_gpu_geometries_with_fewer_wavefronts(name, H, sg, oracle_mod):
    """k_deblock with 8, 2 and 1 wavefronts per picture: 17 macroblock rows are three groups of eight -- three rounds of one wavefront, the plan with two
    buffers in the last ring, which otherwise only 4K pictures reach"""
    kw, case = RECIPES[name], _case(sg, oracle_mod, name)
    wmb, hmb = (kw["width"] + 15) // 16, (kw["height"] + 15) // 16
    for waves in (8, 2, 1):
        out, _, _, bad = _decode(H, kw, case[0], 0, k5_waves=waves)
        _check(name, out, case, "%d wavefronts" % waves)
        assert bad == 0
    if hmb == 17:  # with the default eight wavefronts these pictures are one round of three: only the hook takes them to three rounds
        nw, ring, ring_last, bufs, lds = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        assert H.load_hooks().h264mi_internal_deblock_plan(wmb, hmb, ctypes.byref(nw), ctypes.byref(ring), ctypes.byref(ring_last), ctypes.byref(bufs), ctypes.byref(lds)) == 0
        assert nw.value == 3 and bufs.value == 1


@pytest.mark.gpu
def test_gpu_batch_of_four_recipes(H, sg, oracle_mod):
    """Per-slice filter fields, B pictures, a tall picture of three groups and unequal chroma offsets in ONE batch of one decoder."""
    from test_gpu_parity import _decode_gpu
    names = ["slices3_per_slice_cabac", "b_spatial_cabac", "geo_16x272", "cqp_minus12_high_8x8"]
    cases = [_case(sg, oracle_mod, n) for n in names]
    kws = [RECIPES[n] for n in names]
    for x_wgs in (None, 0):
        out, info = _decode_gpu(H, [c[0] for c in cases], max(k["width"] for k in kws), max(k["height"] for k in kws), max(pictures_of(k) for k in kws),
                                max(k.get("slices", 1) for k in kws), x_wgs=x_wgs)
        for i, n in enumerate(names):
            W, Hc = (kws[i]["width"] + 15) & ~15, (kws[i]["height"] + 15) & ~15
            assert out[i].shape[0] == kws[i]["frames"], n
            assert np.array_equal(out[i][:, :W * Hc * 3 // 2], cases[i][1]), (n, x_wgs)
