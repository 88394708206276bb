"""Random access on the CPU: picture management of a stream that is joined at a recovery point, through the product's host side built against the null
device of tools/hoststub (tools/host_random_access.cpp: kernels are not run).  A stream cut at an entry point must give exactly the pictures of the whole
stream from the entry picture on, minus the leading ones, with the frame_num, the PicOrderCnt (up to one constant) and the reference lists of the whole
stream.  What this cannot show is a single sample -- tests/test_random_access_gpu.py does that on the device."""
import shutil
import subprocess

import pytest

import hostprog
import rautil

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")
NAMES = sorted(rautil.RECIPES)


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return hostprog.build("host_random_access.sh", tmp_path_factory.mktemp("host_ra"))


class Run:
    """What tools/host_random_access printed: per chunk (prepare result, stream status), the frames in decoding order, the stream's counters."""

    def __init__(self, tool, tmp, data, mode, ends=()):
        path = tmp / "in.h264"
        path.write_bytes(data)
        r = subprocess.run([tool, str(path), "176", "144", "64", str(mode)] + [str(e) for e in ends], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        self.text, self.chunks, self.frames, self.totals, self.mode_result = r.stdout, [], [], None, 0
        for line in r.stdout.splitlines():
            kind, rest = line[0], line[2:]
            if kind == "M":
                self.mode_result = int(rest)
            elif kind == "P":
                self.chunks.append(tuple(int(v) for v in rest.split()))
            elif kind == "F":
                a, b = rest.split(" | ")
                fn, poc, ref, idr, newseq, field = (int(v) for v in a.split())
                e = [int(v) for v in b.split()]
                self.frames.append(dict(frame_num=fn, poc=poc, ref=ref, idr=idr, new_sequence=newseq, field_coded=field, rp=tuple(e[:5]), entry=e[5], slices=[]))
            elif kind == "S":
                a, b = rest.split(" | ")
                a, b = [int(v) for v in a.split()], [int(v) for v in b.split()]
                self.frames[-1]["slices"].append(dict(cur=a[1], lists=(a[3:3 + a[2]], b[1:1 + b[0]])))
            elif kind == "T":
                self.totals = tuple(int(v) for v in rest.split())


@pytest.fixture(scope="module")
def whole(tool, tmp_path_factory, sg):
    """Every recipe's whole stream, decoded once with the mode off and once with it on"""
    tmp = tmp_path_factory.mktemp("whole")
    return {name: (Run(tool, tmp, rautil.case(sg, name).stream, 0), Run(tool, tmp, rautil.case(sg, name).stream, 1)) for name in NAMES}


def test_mode_values(tool, tmp_path, sg):
    data = rautil.case(sg, "a").stream
    assert Run(tool, tmp_path, data, 2).mode_result == -1 and Run(tool, tmp_path, data, -1).mode_result == -1
    assert Run(tool, tmp_path, data, 1).mode_result == 0 and Run(tool, tmp_path, data, 0).mode_result == 0


@pytest.mark.parametrize("name", NAMES)
def test_whole_stream_with_the_mode_on(whole, sg, name):
    c, (off, on) = rautil.case(sg, name), whole[name]
    assert off.chunks == on.chunks == [(0, 0)] and len(on.frames) == c.frames
    assert on.totals == off.totals == (0, 0, 0), "a stream that starts at its IDR picture enters nowhere else and skips nothing"
    entry_frames = {e["frame"] for e in c.entries}
    for t, (a, b) in enumerate(zip(off.frames, on.frames)):
        assert b["rp"] == ((1, 0, 1, 0, 0) if t in entry_frames else (0, 0, 0, 0, 0)), t
        assert b["entry"] == (t == 0) and a["entry"] == 0
        assert b["new_sequence"] == (t == 0)
        assert {k: v for k, v in a.items() if k != "entry"} == {k: v for k, v in b.items() if k != "entry"}, "the mode changes nothing else"


def _cuts(c):
    return [(k, kind, en, c.stream[en[kind]:]) for k, en in enumerate(c.entries) for kind in ("cut", "garbage_cut")]


@pytest.mark.parametrize("name", NAMES)
def test_join_at_every_entry_point(tool, tmp_path, whole, sg, name):
    c, ref = rautil.case(sg, name), whole[name][0].frames
    for k, kind, en, data in _cuts(c):
        got = Run(tool, tmp_path, data, 1)
        assert got.chunks == [(0, 0)], (k, kind, got.text[:200])
        want = [ref[t] for t in en["expect"]]
        assert len(got.frames) == len(want), (k, kind)
        assert [f["frame_num"] for f in got.frames] == [f["frame_num"] for f in want]
        assert len({g["poc"] - w["poc"] for g, w in zip(got.frames, want)}) == 1, "PicOrderCnt up to one constant"
        assert [f["entry"] for f in got.frames] == [1] + [0] * (len(want) - 1)
        assert [f["new_sequence"] for f in got.frames] == [1] + [0] * (len(want) - 1)
        assert [(f["ref"], f["idr"], f["field_coded"], f["rp"]) for f in got.frames] == [(f["ref"], f["idr"], f["field_coded"], f["rp"]) for f in want]
        # one non-IDR entry taken (the later recovery points are passed while decoding); the generator's count of leading pictures
        assert got.totals[0] == 1 and got.totals[2] == en["leading"], (k, kind, got.totals)
        # the garbage cut begins inside a slice and with slices before their parameter sets: skipped and counted, never an error
        assert got.totals[1] == (0 if kind == "cut" else 2), "half a slice without a start code, then two whole slices"


@pytest.mark.parametrize("name", [n for n in NAMES if not rautil.RECIPES[n].get("field_pics")])
def test_join_keeps_the_list_indices(tool, tmp_path, whole, sg, name):
    """Every list entry that the whole-stream decode resolves to a picture at or after the entry picture (in decoding order) sits at the same index,
    with the same PicOrderCnt distance, in the decode that joined there.  (h264mi_frame_ref_pocs does not report field pictures: recipes (d), (e).)

    Recipe (c) is the hard one: with num_ref_frames 4 the reference B picture of the group BEFORE the one the entry picture closes (display index 2 when
    the entry picture is 8) is still in the window when the pictures behind the entry picture are decoded, and it lies in front of the entry picture in
    decoding order too.  In RefPicList0 of a B picture -- earlier pictures nearest first, then the later ones -- it stands in front of every later
    picture: the B picture with display index 10 has [8, 6, 2, 12].  A decoder that started at 8 with an empty window would have [8, 6, 12]; the
    non-existing frames that Dpb::start_at_entry puts into the window for the frame_num values in front of the entry picture's keep 12 at index 3."""
    c, ref = rautil.case(sg, name), whole[name][0].frames
    checked = 0
    for k, kind, en, data in _cuts(c):
        got = Run(tool, tmp_path, data, 1)
        poc_to_frame = {f["poc"]: t for t, f in enumerate(ref)}  # (one IDR picture: the counts of the whole stream are unique)
        for g, t in zip(got.frames, en["expect"]):
            assert len(g["slices"]) == len(ref[t]["slices"]) > 0
            for gs, ws in zip(g["slices"], ref[t]["slices"]):
                for l in range(2):
                    assert len(gs["lists"][l]) == len(ws["lists"][l]), "the active size is the slice header's"
                    for i, p in enumerate(ws["lists"][l]):
                        if poc_to_frame.get(p, -1) >= en["frame"] and p != ws["cur"]:  # (an empty place is reported with the picture's own count)
                            print(name, k, kind, "frame", t, "list", l, "index", i, "whole", [q - ws["cur"] for q in ws["lists"][l]], "joined", [q - gs["cur"] for q in gs["lists"][l]])
                            assert gs["lists"][l][i] - gs["cur"] == p - ws["cur"], (k, kind, t, l, i)
                            checked += 1
    assert checked > 0


@pytest.mark.parametrize("name", NAMES)
def test_cut_streams_fail_with_the_mode_off(tool, tmp_path, sg, name):
    for k, kind, en, data in _cuts(rautil.case(sg, name)):
        got = Run(tool, tmp_path, data, 0)
        assert got.chunks == [(-2, -2)] and got.frames == [], (k, kind)  # H264MI_EBITSTREAM, today's behaviour


@pytest.mark.parametrize("name", NAMES)
def test_join_fed_in_chunks(tool, tmp_path, sg, name):
    """The cut stream in chunks: one boundary between the entry picture and its leading pictures, and a boundary at every access unit"""
    c = rautil.case(sg, name)
    for en in c.entries[:2]:
        data = c.stream[en["cut"]:]
        one = Run(tool, tmp_path, data, 1)
        aus = [a for a in rautil.access_unit_starts(data) if a > 0]
        behind_entry = aus[c.pics_per_frame - 1]  # the entry picture is the first access unit (a frame of two fields: the first two)
        for ends in ([behind_entry], aus):
            got = Run(tool, tmp_path, data, 1, ends)
            assert all(ch == (0, 0) for ch in got.chunks) and len(got.chunks) == len(ends) + 1
            assert got.frames == one.frames and got.totals == one.totals, ends[:3]
