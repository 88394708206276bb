"""Regenerates tests/golden/stream_md5.json: MD5 of each synthetic stream of the parity matrix and of
its decoded frames (oracle output, which equals the generator's own reconstruction).  The vectors
pin generator + oracle against silent behavioural drift; they do not come from the reference, which
has no test vectors."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))
import oracle  # noqa: E402
import streamgen  # noqa: E402
from conftest import FIELD_CABAC_MATRIX, FIELD_MATRIX, MATRIX, POC_MATRIX  # noqa: E402

out = {}
for name in sorted(MATRIX):
    s, rec, _ = streamgen.encode(**MATRIX[name])
    frames, _ = oracle.decode(s, crop=False)
    assert (frames == rec).all(), name
    out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(frames.tobytes()).hexdigest(), "stream_bytes": len(s)}
json.dump(out, open(os.path.join(HERE, "stream_md5.json"), "w"), indent=1, sort_keys=True)
print("wrote", len(out), "vectors")

# field pictures (oracle + generator only): their own file, so that the GPU golden test keeps reading stream_md5.json whole
out = {}
for name in sorted(FIELD_MATRIX):
    s, rec, _ = streamgen.encode(**FIELD_MATRIX[name])
    frames, _ = oracle.decode(s, crop=False)
    assert (frames == rec).all(), name
    out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(frames.tobytes()).hexdigest(), "stream_bytes": len(s)}
json.dump(out, open(os.path.join(HERE, "field_md5.json"), "w"), indent=1, sort_keys=True)
print("wrote", len(out), "field vectors")

# the same recipes with CABAC (unpinned context values of field-coded blocks: these vectors pin the mechanism and guard against drift, nothing more)
out = {}
for name in sorted(FIELD_CABAC_MATRIX):
    s, rec, _ = streamgen.encode(**FIELD_CABAC_MATRIX[name])
    frames, _ = oracle.decode(s, crop=False)
    assert (frames == rec).all(), name
    out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(frames.tobytes()).hexdigest(), "stream_bytes": len(s)}
json.dump(out, open(os.path.join(HERE, "field_cabac_md5.json"), "w"), indent=1, sort_keys=True)
print("wrote", len(out), "CABAC field vectors")

# separate bottom-field picture order counts (CPU-checked cases: oracle, generator, and the product's host side against the null device)
out = {}
for name in sorted(POC_MATRIX):
    s, rec, _ = streamgen.encode(**POC_MATRIX[name])
    frames, _ = oracle.decode(s, crop=False)
    assert (frames == rec).all(), name
    out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(frames.tobytes()).hexdigest(), "stream_bytes": len(s),
                 "pocs": [int(x) for x in streamgen.last_pocs()]}
json.dump(out, open(os.path.join(HERE, "poc_md5.json"), "w"), indent=1, sort_keys=True)
print("wrote", len(out), "POC vectors")



def value_range_vectors():
    """tests/rangeutil.py: the recipes at the ends of the value ranges of inter prediction, the vector syntax and the scaling lists."""
    import rangeutil
    out = {}
    for name in sorted(rangeutil.RECIPES):
        s, rec, _ = streamgen.encode(**rangeutil.RECIPES[name])
        pocs = [int(x) for x in streamgen.last_pocs()]
        frames, _ = oracle.decode(s, crop=False)
        assert (frames == rec).all(), name
        out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(rec.tobytes()).hexdigest(), "stream_bytes": len(s), "pocs": pocs}
    json.dump(out, open(os.path.join(HERE, "value_range_md5.json"), "w"), indent=1, sort_keys=True)
    print("wrote", len(out), "value range vectors")


value_range_vectors()


def deblock_vectors():
    """tests/deblockutil.py: the recipes whose deblocking branches are counted, and the geometries k_deblock distinguishes."""
    import deblockutil
    out = {}
    for name in sorted(deblockutil.RECIPES):
        s, rec, _ = streamgen.encode(**deblockutil.RECIPES[name])
        frames, _ = oracle.decode(s, crop=False)
        assert (frames == rec).all(), name
        out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(rec.tobytes()).hexdigest(), "stream_bytes": len(s)}
    json.dump(out, open(os.path.join(HERE, "deblock_md5.json"), "w"), indent=1, sort_keys=True)
    print("wrote", len(out), "deblocking vectors")


deblock_vectors()


def entropy_syntax_vectors():
    """tests/syntaxutil.py: the recipes at the ends of the entropy syntax (streamgen's syntax_stim)."""
    import syntaxutil
    out = {}
    for name in sorted(syntaxutil.RECIPES):
        s, rec, _ = streamgen.encode(**syntaxutil.RECIPES[name])
        pocs = [int(x) for x in streamgen.last_pocs()]
        frames, _ = oracle.decode(s, crop=False)
        assert (frames == rec).all(), name
        out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(rec.tobytes()).hexdigest(), "stream_bytes": len(s), "pocs": pocs}
    json.dump(out, open(os.path.join(HERE, "entropy_syntax_md5.json"), "w"), indent=1, sort_keys=True)
    print("wrote", len(out), "entropy syntax vectors")


entropy_syntax_vectors()


def motion_vectors():
    """tests/motionutil.py: the recipes whose motion derivations are counted cell by cell, and the geometries of the entropy kernels' P paths."""
    import motionutil
    out, lines = {}, []
    for name in sorted(motionutil.RECIPES):
        kw = motionutil.RECIPES[name]
        s, rec, _ = streamgen.encode(**kw)
        pics = motionutil.derive_stream(streamgen.last_motion_trace(), inference=not kw.get("direct_4x4"))
        cells = motionutil.Counter()
        for p in pics:
            cells.update(p.cells)
        lines.append(motionutil.cell_line(name, cells))
        frames, _ = oracle.decode(s, crop=False)
        assert (frames == rec).all(), name
        out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(rec.tobytes()).hexdigest(), "stream_bytes": len(s)}
    json.dump(out, open(os.path.join(HERE, "motion_md5.json"), "w"), indent=1, sort_keys=True)
    open(os.path.join(HERE, "motion_counters.txt"), "w").write(
        "The cells of 8.4.1 that the yardstick of tests/motionutil.py counts on the motion trace of each recipe there, at the seeds chosen there:\n"
        "per family, distinct cells reached / derivations counted.\n" + "\n".join(lines) + "\n")
    print("wrote", len(out), "motion vectors")


motion_vectors()


def intra_vectors():
    """tests/intrautil.py: the recipes whose intra-prediction cells are counted, and the geometries K3's schedules distinguish."""
    import intrautil
    out, lines = {}, []
    for name in sorted(intrautil.RECIPES):
        s, rec, _ = streamgen.encode(**intrautil.RECIPES[name])
        lines.append(intrautil.counter_line(name, streamgen.last_ranges()))
        frames, _ = oracle.decode(s, crop=False)
        assert (frames == rec).all(), name
        out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(rec.tobytes()).hexdigest(), "stream_bytes": len(s)}
    json.dump(out, open(os.path.join(HERE, "intra_md5.json"), "w"), indent=1, sort_keys=True)
    open(os.path.join(HERE, "intra_counters.txt"), "w").write(
        "streamgen.last_ranges() of the recipes of tests/intrautil.py at the seeds chosen there (what met the conditions of intrautil.unmet()).\n"
        "cells = cells reached; 4 / 8 / 16 / c = per prediction mode the mask of availability combinations (left | top << 1 | topleft << 2 | topright << 3);\n"
        "tr4 / tr8 = per block index, modes 3 and 7: 1 real samples above right, 2 substituted, 3 both.\n" + "\n".join(lines) + "\n")
    print("wrote", len(out), "intra vectors")


intra_vectors()


def residual_vectors():
    """tests/residualutil.py: the recipes whose residual decoding (8.5) is counted cell by cell, and the largest dequantised coefficient per class."""
    import residualutil
    out, lines, max_d = {}, [], {}
    for name in sorted(residualutil.RECIPES):
        s, rec, _ = streamgen.encode(**residualutil.RECIPES[name])
        cells = residualutil.Counter()
        for p in residualutil.reconstruct_stream(streamgen.last_residual_trace()):
            cells.update(p.cells)
            for k, v in p.max_d.items():
                max_d[k] = max(max_d.get(k, 0), v)
        lines.append(residualutil.cell_line(name, cells))
        frames, _ = oracle.decode(s, crop=False)
        assert (frames == rec).all(), name
        out[name] = {"stream_md5": hashlib.md5(s).hexdigest(), "frames_md5": hashlib.md5(rec.tobytes()).hexdigest(), "stream_bytes": len(s)}
    json.dump(out, open(os.path.join(HERE, "residual_md5.json"), "w"), indent=1, sort_keys=True)
    open(os.path.join(HERE, "residual_counters.txt"), "w").write(
        "The cells of 8.5 that the yardstick of tests/residualutil.py counts on the residual trace of each recipe there, at the seeds chosen there:\n"
        "per family, distinct cells reached / decisions counted.  T: per class the power of two of residualutil.T and the largest dequantised magnitude\n"
        "the recipes reach together.\n" + "\n".join(lines) + "\n" + residualutil.max_line(max_d) + "\n")
    print("wrote", len(out), "residual vectors")


residual_vectors()

# the characterisation trace of the product's picture management (tests/dpbtrace.py; CPU, null device): MD5 of the trace text of every case.  It
# pins what the code DOES, so it is written once and not again for a change that is meant to keep behaviour.  Only with --dpb-trace.
if "--dpb-trace" in sys.argv[1:]:
    import tempfile

    import dpbtrace  # noqa: E402
    streamgen.build()
    with tempfile.TemporaryDirectory() as tmp:
        prog = dpbtrace.build(tmp)
        out = {name: hashlib.md5(dpbtrace.trace(prog, tmp, *case).encode()).hexdigest() for name, case in dpbtrace.cases(streamgen).items()}
    json.dump(out, open(os.path.join(HERE, "dpb_trace_md5.json"), "w"), indent=1, sort_keys=True)
    print("wrote", len(out), "picture management traces")
