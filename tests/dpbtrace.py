"""The characterisation trace of the product's picture management (tools/host_dpb_trace.cpp: the host side with its test hooks against the null
device): the cases, and how one is run.  Shared by tests/test_host_dpb_trace.py and tests/golden/make_golden.py, which writes the fixture
tests/golden/dpb_trace_md5.json the test holds the traces against."""
import os
import subprocess

import concealutil as cu
import concealutil2 as c2
import hostprog
from conftest import FIELD_CABAC_MATRIX, FULL_MATRIX, pictures_of

SLICES, PICTURES, FIELDS = 1, 2, 4  # H264MI_CONCEAL_*
FIELD_MODES = ("lost", "header")  # of concealutil2.make_fields: what the host sees ("damaged" slices parse like intact ones)


def build(tmp):
    """The program, built into `tmp`."""
    return hostprog.build("host_dpb_trace.sh", tmp)


def cases(sg):
    """name -> (recipe, conceal_errors, [chunk, ...]): one batch per chunk, on one decoder.  A chunk that is a list is a batch of that many
    streams, prepared with isolation on."""
    out = {}
    for name, kw in sorted(FULL_MATRIX.items()):
        stream = sg.encode(want_recon=False, **kw)[0]
        out["full/" + name] = (kw, 0, [stream])
        # two batches, cut at the access-unit boundary nearest the middle (by count): slots held and references decoded by the batch before,
        # and -- field streams with an odd number of frames -- a first field that waits for its second one across the boundary
        aus = c2.access_units(stream)
        out["full_two_batches/" + name] = (kw, 0, [b"".join(aus[:len(aus) // 2]), b"".join(aus[len(aus) // 2:])])
    for name, kw in sorted(FIELD_CABAC_MATRIX.items()):
        out["field_cabac/" + name] = (kw, 0, [sg.encode(want_recon=False, **kw)[0]])
    for name, (kw, lost) in sorted(c2.CASES.items()):
        damaged = c2.lose_pictures(sg.encode(want_recon=False, **kw)[0], lost).damaged
        out["lost_pictures/" + name] = (kw, SLICES | PICTURES | FIELDS, [damaged])
        out["lost_pictures_refused/" + name] = (kw, 0, [damaged])
        # the rollback of a refused stream: [good, refused, good] in two batches -- without concealment the damaged stream, all of it in the first
        # batch, is refused where its frame_num gap shows, with pictures and slices of the batch already placed -- and the same two good streams as
        # [good, good]: the good streams' traces must not tell the two apart (rollback_parts)
        good = _halves(sg.encode(want_recon=False, **kw)[0])
        out["rollback/" + name] = (kw, 0, [[good[0], damaged, good[0]], [good[1], b"", good[1]]])
        out["rollback_pair/" + name] = (kw, 0, [[g, g] for g in good])
    for name, kw in sorted(cu.CONCEAL_MATRIX.items()):
        out["lost_slices/" + name] = (kw, SLICES, [cu.make(sg.encode(want_recon=False, **kw)[0], mode="lost")[0]])
    for name, kw in sorted(c2.FIELD_CASES.items()):
        stream = sg.encode(want_recon=False, **kw)[0]
        for mode in FIELD_MODES:
            out["field_slices_%s/%s" % (mode, name)] = (kw, SLICES | FIELDS, [c2.make_fields(stream, mode=mode)[0]])
    return out


def _halves(stream):
    """The stream as two chunks, cut at the access-unit boundary nearest the middle (by count)."""
    aus = c2.access_units(stream)
    return [b"".join(aus[:len(aus) // 2]), b"".join(aus[len(aus) // 2:])]


def rollback_parts(text):
    """A multi-stream trace as {(batch, stream): text}."""
    out, key = {}, None
    for line in text.splitlines():
        if line.startswith("batch "):
            batch = int(line.split()[1])
        elif line.startswith("stream "):
            key = (batch, int(line.split()[1]))
            out[key] = []
        else:
            out[key].append(line)
    return out


def trace(prog, tmp, kw, conceal, chunks):
    """The program's output for one case."""
    n_streams = len(chunks[0]) if isinstance(chunks[0], list) else 0
    paths = ["-s%d" % n_streams] if n_streams else []
    for i, chunk in enumerate(c for b in chunks for c in (b if n_streams else [b])):
        paths.append(os.path.join(str(tmp), "chunk%d.h264" % i))
        with open(paths[-1], "wb") as f:
            f.write(chunk)
    W, Hc = (kw["width"] + 15) & ~15, (kw["height"] + 15) & ~15
    r = subprocess.run([prog, str(W), str(Hc), str(pictures_of(kw)), str(max(8, cu.nslices(kw))), str(conceal), str(int(bool(kw.get("field_pics") and kw.get("cabac"))))] + paths,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout
