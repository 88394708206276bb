"""Characterisation of the product's picture management (mi_dpb.cpp, and what mi_picture.cpp and mi_batch.cpp make of it: PicDesc / SliceDesc /
BSliceExt, waves, levels, launch lists, output frames) on the CPU: the host side with its test hooks against the null device of tools/hoststub prepares every case of
tests/dpbtrace.py and prints the state h264mi_internal_dpb_trace sees -- reference lists entry by entry, marking state slot by slot, the
POC / frame_num history, refusals with their message.  The MD5 of every trace is held against tests/golden/dpb_trace_md5.json, written once by
tests/golden/make_golden.py: a change of this text is a change of behaviour."""
import hashlib
import json
import os
import re
import shutil

import pytest

import dpbtrace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="g++ not available")


@pytest.fixture(scope="module")
def traces(tmp_path_factory, sg):
    tmp = tmp_path_factory.mktemp("host_dpb_trace")
    prog = dpbtrace.build(tmp)
    return {name: dpbtrace.trace(prog, tmp, *case) for name, case in dpbtrace.cases(sg).items()}


def test_traces_match_the_fixture(traces):
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "dpb_trace_md5.json")))
    assert set(traces) == set(gold)
    bad = [name for name, text in sorted(traces.items()) if hashlib.md5(text.encode()).hexdigest() != gold[name]]
    assert not bad, bad


def _fields(line):
    return dict(t.split("=", 1) for t in line.split()[1:] if "=" in t)


def _list(v):
    return [int(x) for x in v.split(",") if x]


def test_a_refused_stream_leaves_no_trace_in_the_batch(traces):
    """An exact rollback: with [good, refused, good] the good streams' traces -- picture indices, mb_base, the launch lists and levels of the whole
    batch included -- are those of the same two streams prepared as [good, good]."""
    names = [n.split("/", 1)[1] for n in traces if n.startswith("rollback/")]
    assert names
    for name in names:
        three, two = dpbtrace.rollback_parts(traces["rollback/" + name]), dpbtrace.rollback_parts(traces["rollback_pair/" + name])
        assert sorted(three) == [(b, s) for b in (0, 1) for s in (0, 1, 2)] and sorted(two) == [(b, s) for b in (0, 1) for s in (0, 1)], name
        assert any(x.startswith("left status=-") for x in three[0, 1]), name
        for b in (0, 1):
            assert three[b, 0] == two[b, 0] and three[b, 2] == two[b, 1], (name, b)
            assert any(x.startswith("pic ") for x in three[b, 2]), name


def test_traces_are_not_vacuous(traces):
    """Over all cases: long-term and non-existing frames, a field taken out of the reference set on its own, field list entries, B slices with two
    lists, inserted pictures with a concealment reference, a first field that waits across a batch boundary, and a refusal; of the batch's tables a
    level above 0, a wave above 0 with B pictures, a picture whose motion is kept, and a stream refused in a batch of several."""
    lines = [line for text in traces.values() for line in text.splitlines()]
    slots = [_fields(x) for x in lines if x.startswith("slot ")]
    slices = [_fields(x) for x in lines if x.startswith("slice ")]
    pics = [_fields(x) for x in lines if x.startswith("pic ")]
    assert any(s["ref"] == "2" for s in slots)
    assert any(s["nonexisting"] == "1" for s in slots)
    assert any(s["funref"] != "0" for s in slots)
    assert any(s["funref"] != "0" for name, text in traces.items() if "field_mmco1" in name for s in map(_fields, text.splitlines()) if "funref" in s)
    assert any(e & 0x4000 for s in slices for e in _list(s["l0"]) if e >= 0)
    assert any(s["type"] == "1" and _list(s["l0"]) and _list(s["l1"]) for s in slices)
    assert any(p["n_slices"] == "0" and int(p["conceal_ref"]) >= 0 for p in pics)
    assert any(x.startswith("state ") and int(_fields(x)["pend_slot"]) >= 0 for x in lines)
    refusals = [x for x in lines if x.startswith("refused ")]
    assert refusals and all(re.match(r"refused prepare=-\d+ status=-\d+: \S", x) for x in refusals)
    levels = [x.split() for x in lines if x.startswith("level ")]
    assert any(int(x[1]) >= 1 and int(_fields(" ".join(x))["n_slices"]) > 0 and _list(_fields(" ".join(x))["prep"]) for x in levels)
    assert any(int(s["level"]) >= 1 for s in slices)
    assert any(int(x.split()[1]) >= 1 and _list(_fields(x)["b"]) for x in lines if x.startswith("wave "))
    assert any(p["save_col"] == "1" for p in pics)
    assert any(x.startswith("left status=-") and "reference pictures are missing" in x for name, text in traces.items() if name.startswith("rollback/") for x in text.splitlines())
    assert all("reference pictures are missing" in text for name, text in traces.items() if name.startswith("lost_pictures_refused/"))
