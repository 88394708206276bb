"""k_entropy_c, the CABAC-only build of the I/P entropy kernel (k_entropy.hip with MI_ENT_CABAC = 1), and its routing.

CPU part (hipcc cross-compiles for gfx950; the hooks library loads without a GPU): the new kernel keeps the register budget of the general one,
is structurally smaller than the general kernel OF THE SAME TREE (fewer spilled scalar registers, less code), keeps the bit reader and the
arithmetic decoder free of spill traffic, and level 0 of a batch is routed to it exactly when all of its slices are CABAC-coded.

GPU part: streams decoded alone (level 0 on k_entropy_c) and next to a CAVLC stream (level 0 on k_entropy) give the generator's pictures bit
for bit -- there is no tolerance anywhere in this file."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import FIELD_CABAC_MATRIX, MATRIX, pictures_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264decode_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the flags of test_entropy_kernel_budget.py (csrc/Makefile's, device side only, to assembly)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S"]


def _tool():
    spec = importlib.util.spec_from_file_location("ent_spills", os.path.join(ROOT, "tools", "ent_spills.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _kernel_metadata(asm, kernel):
    """The kernel-level keys of `kernel`'s entry of amdhsa.kernels, and its code size."""
    body = asm[asm.index("amdhsa.kernels:"):]
    out, cur = {}, None
    for line in body.splitlines():
        m = re.match(r"^(  - |    )\.(\w+):\s+(.*)$", line)
        if not m:
            if line.startswith("amdhsa.") and not line.startswith("amdhsa.kernels"):
                break
            continue
        if m.group(1) == "  - ":
            cur = {}
        cur[m.group(2)] = m.group(3).strip()
        if m.group(2) == "name":
            out[m.group(3).strip()] = cur
    md = dict(out[kernel])
    md["code_len"] = int(re.search(r"codeLenInByte = (\d+)", asm).group(1))
    return md


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """k_entropy and k_entropy_c with the budget flags, and k_entropy_c once more with line tables: three compiles side by side, once per run."""
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the build needs it too")
    tmp = tmp_path_factory.mktemp("ent_cabac")
    jobs = {"k_entropy": ("k_entropy", []), "k_entropy_c": ("k_entropy_c", []), "k_entropy_c_lines": ("k_entropy_c", ["-gline-tables-only"])}
    procs = {}
    for key, (src, extra) in jobs.items():
        procs[key] = subprocess.Popen([HIPCC] + FLAGS + extra + [os.path.join(CSRC, src + ".hip"), "-o", str(tmp / (key + ".s"))], cwd=CSRC,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = {}
    for key, p in procs.items():
        log = p.communicate()[0].decode(errors="replace")
        assert p.returncode == 0, "%s does not compile:\n%s" % (key, log[-2000:])
        out[key] = open(tmp / (key + ".s")).read()
    return out


def _min_waves():
    own = re.search(r"^#define MI_ENT_MINWAVES (\d+)", open(os.path.join(CSRC, "k_entropy_c.hip")).read(), re.M)
    common = open(os.path.join(CSRC, "k_entropy.hip")).read()
    return int(own.group(1)) if own else int(re.search(r"#ifndef MI_ENT_MINWAVES\s+#define MI_ENT_MINWAVES (\d+)", common).group(1))


def test_cabac_kernel_budget(asm):
    md = _kernel_metadata(asm["k_entropy_c"], "k_entropy_c")
    assert int(md["private_segment_fixed_size"]) == 0, "k_entropy_c spills to scratch: %s" % md
    assert int(md.get("vgpr_spill_count", 0)) == 0, md
    assert md.get("uses_dynamic_stack", "false") == "false", md
    # gfx950: 512 registers per lane and SIMD, shared by the VGPRs and AGPRs of the resident waves, allocated in granules of 8
    regs = int(md["vgpr_count"]) + int(md.get("agpr_count", 0))
    waves = min(8, 512 // (-(-regs // 8) * 8))
    assert _min_waves() == 6, "the CABAC-only kernel is built for the general kernel's six waves"
    assert waves >= _min_waves(), "k_entropy_c: %d registers allow %d waves per SIMD, built for %d" % (regs, waves, _min_waves())


def test_cabac_kernel_is_structurally_smaller_than_the_general_one(asm):
    gen = _kernel_metadata(asm["k_entropy"], "k_entropy")
    cab = _kernel_metadata(asm["k_entropy_c"], "k_entropy_c")
    print("sgpr_spill_count: k_entropy %s, k_entropy_c %s; code bytes: %d, %d" % (gen["sgpr_spill_count"], cab["sgpr_spill_count"], gen["code_len"], cab["code_len"]))
    assert int(cab["sgpr_spill_count"]) < int(gen["sgpr_spill_count"])
    assert cab["code_len"] < gen["code_len"]


def test_cabac_kernel_hot_path_has_no_spill_traffic(asm):
    """No lane read or write of the spill VGPR among the instructions of the bit reader and the CABAC engine (the `@region` lines of
    k_entropy.hip): the per-bin code neither spills nor reloads a scalar register."""
    tool = _tool()
    names = [n for _, n in tool.regions()]
    for want in ("bit reader", "CABAC engine", "cabac_residual", "parse_residual_cabac", "vector prediction and caches", "pskip_fast", "decode_mb", "kernel body"):
        assert want in names, "k_entropy.hip has lost its '// @region %s' line" % want
    text = asm["k_entropy_c_lines"]
    tab, spill_regs, _ = tool.table(text)
    print(tool.render(text))
    md = _kernel_metadata(text, "k_entropy_c")
    if int(md["sgpr_spill_count"]) > 0:
        assert spill_regs, "the assembly does not name its spill VGPR any more: tools/ent_spills.py has to learn the compiler's new note"
    for region in ("bit reader", "CABAC engine"):
        c = tab[region]
        assert c["insts"] > 0, "no instruction is attributed to '%s': the line tables or the region markers are off" % region
        assert c["spills"] == 0 and c["reloads"] == 0, (
            "k_entropy_c: %d spills / %d reloads of scalar registers inside '%s', which runs per bin.  The remedy is NOT to delete this test: run "
            "tools/ent_spills.py on the -gline-tables-only assembly of k_entropy_c.hip, see which region's live values grew (profiles/r08_ent_spills_*.txt has "
            "the table this was written against), and take the pressure out there." % (c["spills"], c["reloads"], region))


def test_entropy_kernel_choice(H):
    f = H.load_hooks().h264mi_internal_entropy_kernel_choice
    I32 = ctypes.c_int32
    f.restype, f.argtypes = I32, [I32, I32, I32]
    GENERAL, FMO, CABAC = 0, 1, 2
    assert f(30, 0, 0) == CABAC and f(1, 0, 0) == CABAC        # all-CABAC
    assert f(255, 1, 0) == GENERAL and f(1, 1, 0) == GENERAL   # one CAVLC slice among CABAC ones
    assert f(0, 7, 0) == GENERAL                               # all-CAVLC
    for n_cabac, n_cavlc in ((5, 0), (0, 5), (3, 2), (0, 0)):  # slice groups, whatever the mode
        assert f(n_cabac, n_cavlc, 1) == FMO
    assert f(0, 0, 0) in (GENERAL, FMO, CABAC)                 # an empty level 0 (B slices only): nothing is launched, any id


# ---------------------------------------------------------------------------------------------------------------- GPU
ROUTE_CASES = ("cabac_I", "cabac_IPP", "pcm_qpjitter_cabac", "high8x8_cabac", "slices_idc_cycle", "multiref_cabac", "sub8x8_heavy",
               "oversized_mbs_cabac_8x8", "mono_cabac_8x8_pcm_wp", "slice_qp_delta")
_gen_cache = {}


def _gen(sg, name, matrix=MATRIX):
    """(stream, rec) of a matrix recipe, generated once per run and left unchanged"""
    if name not in _gen_cache:
        stream, rec, _ = sg.encode(**matrix[name])
        rec.setflags(write=False)
        _gen_cache[name] = (stream, rec)
    return _gen_cache[name]


def _nslices(kw):
    return max(1, kw.get("slices", 1)) * max(1, kw.get("slice_groups", 1))


def _decode(H, items, **cfg):
    """items: [(kw, stream)] decoded as ONE batch; per stream its frames, uncropped (every size here is a multiple of 16)"""
    W = max((kw["width"] + 15) & ~15 for kw, _ in items)
    Hc = max((kw["height"] + 15) & ~15 for kw, _ in items)
    dec = H.Decoder(max_streams=len(items), max_width=W, max_height=Hc, max_frames_per_batch=max(pictures_of(kw) for kw, _ in items),
                    max_slices_per_frame=max(_nslices(kw) for kw, _ in items), max_bitstream_bytes=sum(len(s) for _, s in items) * 2 + (1 << 20), **cfg)
    try:
        dec.decode([s for _, s in items])
        return [dec.read_frames(i, crop=True, size=kw["width"] * kw["height"] * 3 // 2) for i, (kw, _) in enumerate(items)]
    finally:
        dec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROUTE_CASES)
def test_gpu_both_routes_give_the_same_pictures(name, H, sg):
    kw = MATRIX[name]
    assert kw["cabac"] == 1 and kw["width"] <= 176 and kw["height"] <= 144 and 2 <= kw["frames"] <= 6
    stream, rec = _gen(sg, name)
    cav_kw = MATRIX["cavlc_I"]
    cav, cav_rec = _gen(sg, "cavlc_I")
    alone = _decode(H, [(kw, stream)])                      # level 0 all CABAC: k_entropy_c
    assert alone[0].shape == rec.shape and np.array_equal(alone[0], rec), "k_entropy_c != generator reconstruction"
    mixed = _decode(H, [(kw, stream), (cav_kw, cav)])       # one CAVLC slice in the launch: k_entropy
    assert np.array_equal(mixed[0], rec), "k_entropy != generator reconstruction"
    assert np.array_equal(mixed[1], cav_rec), "the CAVLC stream of the mixed batch"


@pytest.mark.gpu
def test_gpu_level0_on_the_cabac_kernel_with_b_slices_behind_it(H, sg):
    kw = MATRIX["b_ibbp_cabac"]
    stream, rec = _gen(sg, "b_ibbp_cabac")
    out = _decode(H, [(kw, stream)])
    assert out[0].shape == rec.shape and np.array_equal(out[0], rec)


@pytest.mark.gpu
def test_gpu_field_cabac_on_request_through_the_cabac_kernel(H, sg):
    """the field scans and significance maps are selected per picture inside the same source"""
    kw = FIELD_CABAC_MATRIX["field_IP_cabac"]
    stream, rec = _gen(sg, "field_IP_cabac", FIELD_CABAC_MATRIX)
    out = _decode(H, [(kw, stream)], allow_unpinned_field_cabac=1)
    assert out[0].shape == rec.shape and np.array_equal(out[0], rec)


@pytest.mark.gpu
def test_gpu_damaged_slice_ends_the_cabac_kernel_in_order(H, sg):
    """One byte of the second picture's slice data flipped, no concealment: the call returns, the stream's status is what the corrupt-stream
    test of test_gpu_parity.py accepts (0: the damage decoded as something, or H264MI_ECORRUPT -8), the intact stream beside it is exact."""
    kw = MATRIX["cabac_IPP"]
    stream, rec = _gen(sg, "cabac_IPP")
    nals = H.read_nal_units(stream)
    slices = [i for i, n in enumerate(nals) if n.Type in (1, 5)]
    second = slices[1]
    begin = nals[second].Offset
    end = nals[second + 1].Offset - 4 if second + 1 < len(nals) else len(stream)
    assert end - begin > 64
    b = bytearray(stream)
    b[begin + (end - begin) // 2] ^= 0xFF
    good_kw = MATRIX["cabac_I"]
    good, good_rec = _gen(sg, "cabac_I")
    dec = H.Decoder(max_streams=2, max_width=176, max_height=144, max_frames_per_batch=kw["frames"], max_bitstream_bytes=1 << 20)
    try:
        dec.set_isolation(True)
        dec.decode([bytes(b), good])
        status = dec.stream_status(0)
        print("status of the damaged stream: %d" % status)
        assert status in (0, -8)
        assert dec.stream_status(1) == 0
        assert np.array_equal(dec.read_frames(1, crop=True, size=good_kw["width"] * good_kw["height"] * 3 // 2), good_rec)
        assert np.array_equal(dec.read_frames(0, crop=False)[0], rec[0]), "the intact first picture of the damaged stream"
    finally:
        dec.close()
