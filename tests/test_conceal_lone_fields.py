"""Error concealment of wholly lost FIELDS (h264mi_config.conceal_errors with H264MI_CONCEAL_LONE_FIELDS): a frame coded as two field pictures of which
one never arrives is completed with an inserted field, a zero-motion copy of entry 0 of that field's initial P list (8.2.4.2.5), in front of whatever
shows that the field is missing.  The yardstick is the oracle's decode of the REPAIRED stream (tests/concealutil4.py); every GPU comparison is
bit-exact."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import concealutil as cu
import concealutil2 as c2
import concealutil4 as c4
import dpbtrace
from concealutil4 import FIELDS, LONE, LONE_CASES, PICTURES, SLICES
from conftest import FIELD_MATRIX, pictures_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HF = 176, 128  # coded size of every case
REF_PARITY = 1 << 14  # MI_REF_PARITY: the bottom field of a frame slot in a list entry


def _bits(name):
    return SLICES | FIELDS | LONE | (PICTURES if LONE_CASES[name][2] else 0)


def _unpinned(kw):
    return int(bool(kw.get("field_pics") and kw.get("cabac")))


_cache = {}


def _case(name, sg, oracle_mod):
    """(recipe, original stream, Lone, oracle frames of the repaired stream, its PicOrderCnt list), computed once."""
    if name not in _cache:
        kw, stream, r = c4.build_case(name, sg)
        want, _ = oracle_mod.decode(r.repaired, crop=False)
        want.setflags(write=False)
        _cache[name] = (kw, stream, r, want, [int(x) for x in oracle_mod.last_pocs])
    return _cache[name]


# ---------------------------------------------------------------- CPU: the writer and the rule, independent of the product's device code
def test_the_matrix_has_the_required_shapes(sg):
    c4.check_recipes()
    c4.check_matrix({name: c4.build_case(name, sg)[2] for name in LONE_CASES})


@pytest.mark.parametrize("name", sorted(LONE_CASES))
def test_repaired_stream_is_a_valid_stream(name, sg, oracle_mod):
    """The oracle decodes the repaired stream: the frame count of the original, the frames in front of the first loss untouched, and every inserted
    field equal to the field the rule names -- entry 0 of its initial P list for fields, taken from the oracle's own output frames.  Luma always; chroma
    when that field has the parity of the inserted one (a zero luma vector into a field of the other parity is a chroma vector of a quarter sample,
    8.4.1.4: there the chroma rows are interpolated, and only their difference from grey is asserted)."""
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    c4.check_case(r)
    ref, info = oracle_mod.decode(stream, crop=False)
    assert len(want) == info.n_frames == kw["frames"] == len(r.frames) == len(pocs)
    ft = r.first_touched()
    assert np.array_equal(want[:ft], ref[:ft])
    n = 0
    for i, f in enumerate(r.frames):
        for ins in f["inserted"]:
            j, par = ins["copy_of"]
            assert j < i or (j == i and par != ins["parity"])
            mine, src = c4.parity_rows(want[i], W, HF, ins["parity"]), c4.parity_rows(want[j], W, HF, par)
            assert np.array_equal(mine[0], src[0]), (i, ins)
            assert not (mine[0] == 128).all()
            if par == ins["parity"] or kw.get("mono"):
                assert np.array_equal(mine[1], src[1]) and np.array_equal(mine[2], src[2]), (i, ins)
            n += 1
    assert n == r.n_inserted() >= 2
    if name == "with_lost_frame_cavlc_refs2":  # pictures 6 and 7 are the two fields of the frame with frame_num 3: one frame is inserted for them
        assert [f["frame_num"] for f in r.frames if f["whole"]] == [3]
    else:
        assert not any(f["whole"] for f in r.frames)


# ---------------------------------------------------------------- CPU: the product's host side against the null device
@pytest.fixture(scope="module")
def tracer(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    tmp = tmp_path_factory.mktemp("dpb_trace_lone")
    return dpbtrace.build(tmp), tmp


def _trace(prog, tmp, kw, conceal, chunks, frames=None):
    """dpbtrace.trace with the decoder's max_frames_per_batch given: by default two pictures per frame, no headroom."""
    paths = []
    for i, chunk in enumerate(chunks):
        paths.append(os.path.join(str(tmp), "lone%d.h264" % i))
        with open(paths[-1], "wb") as f:
            f.write(chunk)
    res = subprocess.run([prog, str(W), str(HF), str(frames or pictures_of(kw)), str(max(8, cu.nslices(kw))), str(conceal), str(_unpinned(kw))] + paths,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout


def _parse_trace(text):
    pics, outs = {}, []
    for line in text.splitlines():
        kv = dict(x.split("=", 1) for x in line.split()[1:] if "=" in x)
        if line.startswith("pic "):
            pics[int(line.split()[1])] = {k: int(v) for k, v in kv.items() if k in ("slot", "field", "wave", "conceal_ref", "n_slices", "frame_num")}
        elif line.startswith("out "):
            outs.append({k: int(v) for k, v in kv.items() if k in ("slot", "poc", "frame_num", "pic", "pic2", "nal_ref_idc", "idr")})
    return pics, outs


@pytest.mark.parametrize("name", sorted(LONE_CASES))
def test_host_inserts_the_missing_fields(name, tracer, sg, oracle_mod):
    """Picture management alone (no GPU), one batch: the frame_num / PicOrderCnt list of the damaged stream is the oracle's for the repaired stream;
    every inserted field is a picture without slices of the right parity, in its frame's slot, whose concealment reference is the slot and parity the
    rule names and whose wave is behind that picture's; nothing else is without slices.  With the bit clear no picture is inserted."""
    prog, tmp = tracer
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    pics, outs = _parse_trace(_trace(prog, tmp, kw, _bits(name), [r.damaged]))
    assert [o["poc"] for o in outs] == pocs
    assert [o["frame_num"] for o in outs] == [f["frame_num"] for f in r.frames]
    assert [o["nal_ref_idc"] != 0 for o in outs] == [f["ref"] for f in r.frames]
    assert len({o["slot"] for o in outs}) == len(outs)  # (one batch: a slot taken by a picture of the batch stays taken)
    expected = set()
    for i, f in enumerate(r.frames):
        for ins in f["inserted"]:
            q = outs[i]["pic2"]
            pd = pics[q]
            expected.add(q)
            assert pd["n_slices"] == 0 and pd["field"] == 1 + ins["parity"] and pd["slot"] == outs[i]["slot"], (i, pd)
            j, par = ins["copy_of"]
            assert pd["conceal_ref"] == outs[j]["slot"] | (REF_PARITY if par else 0), (i, pd, outs[j])
            src = [p for p in (outs[j]["pic"], outs[j]["pic2"]) if p >= 0 and pics[p]["field"] in (0, 1 + par)]
            assert len(src) == 1 and pd["wave"] > pics[src[0]]["wave"], (i, pd, src)
        if f["whole"]:
            expected.add(outs[i]["pic"])
            assert pics[outs[i]["pic"]]["n_slices"] == 0 and pics[outs[i]["pic"]]["field"] == 0
    assert {q for q, pd in pics.items() if pd["n_slices"] == 0} == expected
    if not LONE_CASES[name][2]:
        text = _trace(prog, tmp, kw, SLICES | FIELDS, [r.damaged])
        if name == "mixed_paff_cavlc_refs3":  # (a frame picture behind a lone IDR field has no reference frame to predict from)
            assert "refused" in text and "without reference pictures" in text
        else:
            pics0, outs0 = _parse_trace(text)
            assert "refused" not in text and all(pd["n_slices"] > 0 for pd in pics0.values()) and len(outs0) == len(outs)


def test_host_keeps_to_the_room_of_the_batch(tracer, sg, oracle_mod):
    """One access unit per batch.  With room for two pictures the field is inserted in front of the revealing picture, in ITS batch, and refers to a
    slot that an earlier batch decoded (wave 0); with room for one picture it is not, and the frame goes out as with the bit clear."""
    prog, tmp = tracer
    name = "idr_second_cavlc_refs2_idc0"
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    aus = c2.access_units(r.damaged)
    for room, inserted in ((2, r.n_inserted()), (1, 0)):
        got, n_out = 0, 0
        for batch in _trace(prog, tmp, kw, _bits(name), aus, frames=room).split("batch ")[1:]:
            pics, outs = _parse_trace(batch)
            n_out += len(outs)
            for pd in pics.values():
                if pd["n_slices"] == 0:
                    got += 1
                    assert pd["wave"] == 0 and pd["conceal_ref"] >= 0 and len(pics) == 2
        assert got == inserted and n_out == len(r.frames), room


def _summary(text):
    """(refused, inserted fields, inserted frames, output frames) of a trace, over all its batches."""
    fields = frames = n_out = 0
    for batch in text.split("batch ")[1:]:
        pics, outs = _parse_trace(batch)
        n_out += len(outs)
        fields += sum(pd["n_slices"] == 0 and pd["field"] != 0 for pd in pics.values())
        frames += sum(pd["n_slices"] == 0 and pd["field"] == 0 for pd in pics.values())
    return "refused" in text, fields, frames, n_out


def _unit_of_type(stream, t):
    return next(u for u in cu.split_units(stream) if c4._nal_type(u) == t)


@pytest.mark.parametrize("which", [7, 8])
def test_host_replaced_parameter_sets_keep_the_grey_rows(which, tracer, sg, oracle_mod):
    """Between the lone IDR field and the revealing picture the SPS (7) / PPS (8) the field was decoded under is stored with other content -- and then
    with the old content again, so that the rest of the stream is what it was: that field is not inserted (the frame goes out as with the bit
    clear), the later lone field is, nothing is refused.  A parameter set that is merely sent again changes nothing."""
    prog, tmp = tracer
    name = "idr_second_cavlc_refs2_idc0"
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    units, _, pics = cu.parse(r.damaged)
    rev = min(s.unit for s in pics[1])  # the picture that reveals that the IDR field is lone
    mine = _unit_of_type(r.damaged, which)
    other = _unit_of_type(sg.encode(want_recon=False, **dict(kw, frames=1, **({"num_ref_frames": 3} if which == 7 else {"chroma_qp_offset": 3})))[0], which)
    assert other != mine
    for between, inserted in ((mine, r.n_inserted()), (other + mine, r.n_inserted() - 1)):
        text = _trace(prog, tmp, kw, _bits(name), [b"".join(units[:rev]) + between + b"".join(units[rev:])])
        assert _summary(text) == (False, inserted, 0, len(r.frames)), (which, between == mine)


def test_host_change_of_sequence_sends_the_lone_field_out(tracer, sg, oracle_mod):
    """A stream that ends in a lone first field, then a sequence of another picture size: its SPS replaces the one the field was decoded under, so the
    frame goes out with the grey rows in front of the new sequence, as with the bit clear, and the new sequence decodes."""
    prog, tmp = tracer
    name = "idr_second_cavlc_refs2_idc0"
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    units, _, pics = cu.parse(stream)
    head = b"".join(units[:min(s.unit for s in pics[3])])  # pictures 0, 1 and 2: a frame and the first field of the next
    tail = sg.encode(want_recon=False, **dict(kw, width=160, height=96, frames=2))[0]
    for bits in (_bits(name), SLICES | FIELDS):
        assert _summary(_trace(prog, tmp, kw, bits, [head + tail])) == (False, 0, 0, 4), bits
    # (the same head in front of an end-of-sequence unit: the field is inserted)
    assert _summary(_trace(prog, tmp, kw, _bits(name), [head + c4.EOS])) == (False, 1, 0, 2)


def test_host_lone_field_and_frame_num_gap_share_the_room(tracer, sg):
    """Bits 2 and 64 together: the second field of a frame and BOTH fields of the next one are lost, so the revealing picture shows a lone field and
    a frame_num gap at once.  One access unit per batch: with room for two pictures the frame inserted for the gap and the revealing picture fill the
    batch, as with bit 64 clear, and the field is not inserted (it must not take the room and turn a concealed gap into a refused stream); with
    room for three both are inserted."""
    prog, tmp = tracer
    kw = LONE_CASES["with_lost_frame_cavlc_refs2"][0]
    units, _, pics = cu.parse(sg.encode(want_recon=False, **kw)[0])
    assert pics[5][0].hdr.frame_num == 2 and pics[6][0].hdr.frame_num == pics[7][0].hdr.frame_num == 3 and pics[8][0].hdr.frame_num == 4
    gone = {s.unit for p in (5, 6, 7) for s in pics[p]}
    aus = c2.access_units(b"".join(u for i, u in enumerate(units) if i not in gone))
    assert len(aus) == len(pics) - 3
    both = SLICES | PICTURES | FIELDS | LONE
    assert _summary(_trace(prog, tmp, kw, SLICES | PICTURES | FIELDS, aus, frames=2)) == (False, 0, 1, kw["frames"])
    assert _summary(_trace(prog, tmp, kw, both, aus, frames=2)) == (False, 0, 1, kw["frames"])
    assert _summary(_trace(prog, tmp, kw, both, aus, frames=3)) == (False, 1, 1, kw["frames"])


def test_abi_has_the_bit_and_the_counter(H):
    """The bit and h264mi_decoder_concealed_fields are in the header, exported, bound in Python and called in Go, the front-ends have the flag, and
    h264mi_decoder_create takes 69, 71, 85 and 87 and refuses the bit without bits 1 and 4 before it looks for a device."""
    from h264decode_amd import _lib
    header = open(os.path.join(ROOT, "include", "h264mi.h")).read()
    assert re.search(r"#define H264MI_CONCEAL_LONE_FIELDS 64\b", header)
    assert re.search(r"int32_t h264mi_decoder_concealed_fields\(h264mi_decoder \*\w*, int64_t \*\w*\);", header)
    L = H.lib()
    assert hasattr(L, "h264mi_decoder_concealed_fields") and "h264mi_decoder_concealed_fields" in _lib.EXPORTS
    assert L.h264mi_decoder_concealed_fields(None, None) == -1
    assert H.CONCEAL_LONE_FIELDS == 64 and hasattr(H.Decoder, "concealed_fields")
    go = open(os.path.join(ROOT, "go", "h264", "h264mi.go")).read()
    assert "C.h264mi_decoder_concealed_fields(" in go and "C.H264MI_CONCEAL_LONE_FIELDS" in go
    example = open(os.path.join(ROOT, "examples", "h264mi_decode.c")).read()
    assert "--conceal-lone-fields" in example and "h264mi_decoder_concealed_fields(" in example and "H264MI_CONCEAL_LONE_FIELDS" in example
    assert "--conceal-lone-fields" in open(os.path.join(ROOT, "tools", "serve.py")).read()
    assert [f for f, _ in _lib.Config._fields_][-1] == "conceal_errors"

    def create(value):
        cfg = _lib.Config()
        cfg.struct_size = ctypes.sizeof(cfg)
        cfg.max_streams, cfg.max_width, cfg.max_height, cfg.max_frames_per_batch, cfg.conceal_errors = 1, 64, 64, 4, value
        h = ctypes.c_void_p()
        code = L.h264mi_decoder_create(ctypes.byref(cfg), ctypes.byref(h))
        text = L.h264mi_last_error_string() if code else b""
        if h:
            L.h264mi_decoder_destroy(h)
        return code, text
    for good in (69, 71, 85, 87):
        code, text = create(good)
        assert code in (0, -4) and b"conceal_errors" not in text, (good, code, text)  # (-4: no device on this machine -- the value was accepted)
    for bad in (64, 65, 66, 68, 72, 128, 8, 9, 24, 25, 32, 33):
        code, text = create(bad)
        assert code == -1 and b"conceal_errors" in text, (bad, code, text)


# ---------------------------------------------------------------- GPU
class _x_wgs:
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = os.environ.get("H264MI_X_WGS")
        if self.n is not None:
            os.environ["H264MI_X_WGS"] = str(self.n)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("H264MI_X_WGS", None)
        else:
            os.environ["H264MI_X_WGS"] = self.old


def _decoder(H, kw, streams, frames=None, **cfg):
    return H.Decoder(max_streams=len(streams), max_width=W, max_height=HF, max_frames_per_batch=frames or pictures_of(kw), max_slices_per_frame=max(cu.nslices(kw), 1),
                     max_bitstream_bytes=sum(len(s) for s in streams) * 2 + (1 << 20), allow_unpinned_field_cabac=_unpinned(kw),
                     b_pictures=int(bool(kw.get("bframes"))), **cfg)  # (single access units: the motion of every reference picture is kept from the start)


def _feed(H, kw, chunks, conceal, frames=None, pipelined=False):
    """One batch per chunk on one decoder: (frames, [(PicOrderCnt, frame_num)], concealed macroblocks per frame, (concealed(), fields, pictures))."""
    dec = _decoder(H, kw, [b"".join(chunks)], frames=frames, conceal_errors=conceal)
    got, infos, mbs = [], [], []
    try:
        def harvest():
            assert dec.stream_status(0) == 0
            n = dec.frame_count(0)
            if n:
                got.extend(f.copy() for f in dec.read_frames(0, crop=False))
            for f in range(n):
                fi = dec.frame_info(0, f)
                infos.append((fi.pic_order_cnt, fi.frame_num))
                mbs.append(dec.frame_concealed(0, f))
        if pipelined:  # execute(k); prepare(k + 1); sync: two batches in flight
            dec.prepare([chunks[0]])
            for k in range(len(chunks)):
                dec.execute()
                if k + 1 < len(chunks):
                    dec.prepare([chunks[k + 1]])
                dec.sync()
                harvest()
        else:
            for c in chunks:
                dec.decode([c])
                harvest()
        return got, infos, mbs, (dec.concealed(), dec.concealed_fields(), dec.concealed_pictures())
    finally:
        dec.close()


def _assert_concealed(res, r, want, pocs, n_pairs, what):
    got, infos, mbs, totals = res
    assert len(got) == len(want), what
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    assert not bad, "%s: frames %r differ from the oracle's decode of the repaired stream" % (what, bad)
    assert [x[0] for x in infos] == pocs and [x[1] for x in infos] == [f["frame_num"] for f in r.frames], what
    assert mbs == r.per_frame(), what
    assert totals == ((0, sum(r.per_frame())), r.n_inserted(), n_pairs), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LONE_CASES))
def test_gpu_lone_fields_are_concealed(name, H, sg, oracle_mod):
    """Every case of the matrix, in the three kernel plans: Y, Cb and Cr of every frame as the oracle decodes the repaired stream, the counters as the
    yardstick's model says."""
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    c4.check_case(r)
    for x in (None, 0, 512):
        with _x_wgs(x):
            _assert_concealed(_feed(H, kw, [r.damaged], _bits(name)), r, want, pocs, len(LONE_CASES[name][2]) // 2, "H264MI_X_WGS=%r" % (x,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["consecutive_cabac_poc1_refs2", "b_cavlc_refs2", "mono_cavlc_poc2_eos", "mixed_paff_cavlc_refs3"])
def test_gpu_single_access_units_pipelined(name, H, sg, oracle_mod):
    """One access unit per prepare, two batches in flight: every lone field was decoded by an earlier batch than the one its complement lands in."""
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    aus = c2.access_units(r.damaged)
    assert len(aus) == len(c2.access_units(stream)) - r.n_lost
    _assert_concealed(_feed(H, kw, aus, _bits(name), frames=2, pipelined=True), r, want, pocs, 0, "pipelined")


@pytest.mark.gpu
def test_gpu_revealing_picture_opens_the_next_batch(H, sg, oracle_mod):
    """The lone field is the last picture of its chunk: its complement opens the next batch, in front of the revealing picture.  And a chunk that holds
    nothing but the end-of-sequence unit: a batch without slices whose only picture is the inserted field."""
    name = "consecutive_cabac_poc1_refs2"
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    aus = c2.access_units(r.damaged)  # pictures 0 1 2 | 4 6 7 8 10 11
    for pipelined in (False, True):
        _assert_concealed(_feed(H, kw, [b"".join(aus[:3]), b"".join(aus[3:])], _bits(name), pipelined=pipelined), r, want, pocs, 0, "two chunks")
    name = "eos_cabac_wp2_refs2"
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    assert r.damaged.endswith(c4.EOS)
    for pipelined in (False, True):
        _assert_concealed(_feed(H, kw, [r.damaged[:-len(c4.EOS)], c4.EOS], _bits(name), pipelined=pipelined), r, want, pocs, 0, "end of sequence alone")


# Without the inserted field a reference list of a later field can come up short (the encoder counted on the lost field), and a macroblock that names
# the missing entry is outside what the standard defines: there the product and the oracle need not agree on the DAMAGED stream.  The cases whose
# lists stay full, where the oracle's decode of the damaged stream is the yardstick of the bit clear for every frame:
FULL_LISTS = ("first_field_cavlc_refs3_idc2",)


def _assert_grey(got, r, want, grey, name, what):
    """What the bit clear means.  The frames in front of the first lone field are untouched; the first frame with a lone field is the oracle's frame
    of the REPAIRED stream with the rows of the field that never came written over with mid-grey, here, in numpy (its first field is decoded from
    intact pictures either way); the rows of every field that never came are mid-grey in every plane; and where no list comes up short every frame
    is the oracle's decode of the damaged stream, which paints the frame store the same way."""
    assert len(got) == len(want) == len(grey), (name, what)
    ft = r.first_touched()
    assert all(np.array_equal(got[i], want[i]) for i in range(ft)), (name, what)
    expect = np.array(want[ft])
    for plane in c4.parity_rows(expect, W, HF, r.frames[ft]["inserted"][0]["parity"]):
        plane[:] = 128  # (views into `expect`)
    assert np.array_equal(got[ft], expect) and not np.array_equal(got[ft], want[ft]), (name, what)
    for i, f in enumerate(r.frames):
        for ins in f["inserted"]:
            assert all((plane == 128).all() for plane in c4.parity_rows(got[i], W, HF, ins["parity"])), (name, what, i)
            assert not (c4.parity_rows(got[i], W, HF, 1 - ins["parity"])[0] == 128).all()
    if name in FULL_LISTS:
        assert all(np.array_equal(a, b) for a, b in zip(got, grey)), (name, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["idr_second_cavlc_refs2_idc0", "second_top_cabac_bff_wp1_ref1_idc1", "first_field_cavlc_refs3_idc2"])
def test_gpu_without_room_in_the_batch_the_rows_stay_grey(name, H, sg, oracle_mod):
    """One access unit per batch and room for ONE picture: the inserted field and the revealing picture do not fit, so the output is, frame for frame,
    what the bit clear gives for the same feed -- the rows of the missing field mid-grey, later fields predicted from them --, the status stays OK
    and nothing is counted.  With room for two the same feed is concealed."""
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    grey, _ = oracle_mod.decode(r.damaged, crop=False)
    aus = c2.access_units(r.damaged)
    off = _feed(H, kw, aus, SLICES | FIELDS, frames=1)
    on = _feed(H, kw, aus, _bits(name), frames=1)
    assert len(on[0]) == len(off[0]) and all(np.array_equal(a, b) for a, b in zip(on[0], off[0]))
    assert on[1:] == off[1:] and on[3] == ((0, 0), 0, 0) and not any(on[2])
    _assert_grey(on[0], r, want, grey, name, "no room")
    _assert_concealed(_feed(H, kw, aus, _bits(name), frames=2), r, want, pocs, 0, "room for two")


@pytest.mark.gpu
@pytest.mark.parametrize("conceal", [SLICES | FIELDS, SLICES | PICTURES | FIELDS])
def test_gpu_bit_clear_keeps_the_grey_rows(conceal, H, sg, oracle_mod):
    """Values 5 and 7 on the damaged streams: the frame goes out with the rows of the missing field mid-grey, as before the bit existed."""
    for name in ("idr_second_cavlc_refs2_idc0", "second_top_cabac_bff_wp1_ref1_idc1", "mono_cavlc_poc2_eos") + FULL_LISTS:
        kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
        grey, _ = oracle_mod.decode(r.damaged, crop=False)
        got, infos, mbs, totals = _feed(H, kw, [r.damaged], conceal)
        _assert_grey(got, r, want, grey, name, conceal)
        assert totals == ((0, 0), 0, 0) and not any(mbs), name


@pytest.mark.gpu
def test_gpu_clean_field_streams_with_the_bit_set(H, sg):
    """Every case of the field matrix decodes exactly with all bits set and reports nothing."""
    for name in sorted(FIELD_MATRIX):
        kw = FIELD_MATRIX[name]
        stream, rec, _ = sg.encode(**kw)
        dec = H.Decoder(max_streams=1, max_width=(kw["width"] + 15) & ~15, max_height=(kw["height"] + 15) & ~15, max_frames_per_batch=pictures_of(kw),
                        max_slices_per_frame=max(cu.nslices(kw), 1), max_bitstream_bytes=len(stream) * 2 + (1 << 20), conceal_errors=SLICES | PICTURES | FIELDS | LONE)
        try:
            dec.decode([stream])
            assert np.array_equal(dec.read_frames(0, crop=False), rec), name
            assert dec.concealed() == (0, 0) and dec.concealed_pictures() == 0 and dec.concealed_fields() == 0, name
            assert all(dec.frame_concealed(0, f) == 0 for f in range(dec.frame_count(0))), name
        finally:
            dec.close()


@pytest.mark.gpu
def test_gpu_one_damaged_stream_among_intact_ones(H, sg, oracle_mod):
    name = "first_field_cavlc_refs3_idc2"
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    others = [dict(cu.CONCEAL_MATRIX["cabac_wp1_multiref"], height=128, frames=6), FIELD_MATRIX["field_bottom_first"], LONE_CASES["b_cavlc_refs2"][0]]
    streams = [sg.encode(want_recon=False, **k)[0] for k in others]
    wants = [oracle_mod.decode(s, crop=False)[0] for s in streams]
    feed, wants = streams[:1] + [r.damaged] + streams[1:], wants[:1] + [want] + wants[1:]
    dec = H.Decoder(max_streams=4, max_width=W, max_height=HF, max_frames_per_batch=15, max_slices_per_frame=4, max_bitstream_bytes=1 << 21, conceal_errors=_bits(name))
    try:
        dec.decode(feed)
        for i in range(4):
            assert dec.stream_status(i) == 0 and dec.frame_count(i) == len(wants[i])
            assert np.array_equal(dec.read_frames(i, crop=False), wants[i]), "stream %d" % i
        assert [dec.frame_concealed(1, f) for f in range(len(want))] == r.per_frame()
        assert dec.concealed() == (0, sum(r.per_frame())) and dec.concealed_fields() == r.n_inserted() and dec.concealed_pictures() == 0
    finally:
        dec.close()


@pytest.mark.gpu
def test_gpu_c_program_with_conceal_lone_fields(H, sg, oracle_mod, tmp_path):
    """examples/h264mi_decode.c --conceal-lone-fields, four pictures per batch: the oracle's frames of the repaired stream, and the field total."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    name = "idr_second_cavlc_refs2_idc0"
    kw, stream, r, want, pocs = _case(name, sg, oracle_mod)
    want_c, info = oracle_mod.decode(r.repaired, crop=True)
    src, dst = tmp_path / "in.h264", tmp_path / "out.yuv"
    src.write_bytes(r.damaged)
    p = subprocess.run([os.path.join(ROOT, "examples", "h264mi_decode"), str(src), str(dst), "4", "--conceal-lone-fields"], stderr=subprocess.PIPE, check=True, timeout=120)
    got = np.frombuffer(dst.read_bytes(), dtype=np.uint8).reshape(-1, info.width * info.height * 3 // 2)
    assert np.array_equal(got, want_c)
    err = p.stderr.decode()
    assert ("concealed: %d fields" % r.n_inserted()) in err and ("concealed: 0 slices, %d macroblocks" % sum(r.per_frame())) in err and "concealed: 0 pictures" in err
