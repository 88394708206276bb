"""k_entropy_m, the Main build of the I/P entropy kernel (k_entropy.hip with MI_ENT_CABAC = 1 and MI_ENT_MAIN = 1: CABAC, no 8x8 transform and
4:2:0 as constants), and its routing.

CPU only (hipcc cross-compiles for gfx950; the hooks library loads without a GPU): the kernel keeps the register budget of the other builds, is
structurally smaller than k_entropy_c OF THE SAME TREE -- fewer spilled scalar registers, less code, no region of the source with more spill
traffic -- keeps the per-bin and per-block code free of spill traffic, and level 0 of a batch is routed to it exactly when all of its slices
are CABAC-coded, no picture has slice groups and no picture of the batch has the 8x8 transform switched on or is monochrome.  No absolute
figure is fixed here: the measured ones are in profiles/ent_main.txt.  (The pictures are in test_entropy_main_gpu.py.)"""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264decode_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the flags of test_entropy_cabac_kernel.py (csrc/Makefile's, device side only, to assembly)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
PER_BIN_REGIONS = ("bit reader", "CABAC engine", "cabac_residual", "parse_residual_cabac")


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
    """k_entropy_c and k_entropy_m with the budget flags, and both once more with line tables: four compiles side by side, once per run."""
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the build needs it too")
    tmp = tmp_path_factory.mktemp("ent_main")
    jobs = {"k_entropy_c": ("k_entropy_c", []), "k_entropy_m": ("k_entropy_m", []),
            "k_entropy_c_lines": ("k_entropy_c", ["-gline-tables-only"]), "k_entropy_m_lines": ("k_entropy_m", ["-gline-tables-only"])}
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
    own = re.search(r"^#define MI_ENT_MINWAVES (\d+)", open(os.path.join(CSRC, "k_entropy_m.hip")).read(), re.M)
    common = open(os.path.join(CSRC, "k_entropy.hip")).read()
    return int(own.group(1)) if own else int(re.search(r"#ifndef MI_ENT_MINWAVES\s+#define MI_ENT_MINWAVES (\d+)", common).group(1))


def test_main_kernel_budget(asm):
    md = _kernel_metadata(asm["k_entropy_m"], "k_entropy_m")
    assert int(md["private_segment_fixed_size"]) == 0, "k_entropy_m spills to scratch: %s" % md
    assert int(md.get("vgpr_spill_count", 0)) == 0, md
    assert md.get("uses_dynamic_stack", "false") == "false", md
    # gfx950: 512 registers per lane and SIMD, shared by the VGPRs and AGPRs of the resident waves, allocated in granules of 8
    regs = int(md["vgpr_count"]) + int(md.get("agpr_count", 0))
    waves = min(8, 512 // (-(-regs // 8) * 8))
    assert _min_waves() == 6, "the Main kernel is built for the six waves of the other builds"
    assert waves >= 6, "k_entropy_m: %d registers allow %d waves per SIMD, built for six" % (regs, waves)


def test_main_kernel_is_structurally_smaller_than_the_cabac_one(asm):
    cab = _kernel_metadata(asm["k_entropy_c"], "k_entropy_c")
    main = _kernel_metadata(asm["k_entropy_m"], "k_entropy_m")
    print("sgpr_spill_count: k_entropy_c %s, k_entropy_m %s; code bytes: %d, %d" % (cab["sgpr_spill_count"], main["sgpr_spill_count"], cab["code_len"], main["code_len"]))
    assert int(main["sgpr_spill_count"]) < int(cab["sgpr_spill_count"])
    assert main["code_len"] < cab["code_len"]


def test_main_kernel_spill_traffic_by_region(asm):
    """Lane writes and reads of the spill VGPR per region of k_entropy.hip (tools/ent_spills.py): none in the code that runs per bin and per
    residual block; in every other region at most as many as k_entropy_c has there (a region's count is its spills plus its reloads); fewer
    in total, the instructions without a source line included.  Measured when this was written: decode_mb 28 against 36, kernel body 39 against
    41, caches and pskip_fast 2 + 2 against 2 + 2, without a source line 5 against 1, 76 against 82 in all."""
    tool = _tool()
    tab_c, regs_c, _ = tool.table(asm["k_entropy_c_lines"])
    tab_m, regs_m, _ = tool.table(asm["k_entropy_m_lines"])
    print("k_entropy_c\n" + tool.render(asm["k_entropy_c_lines"]))
    print("k_entropy_m\n" + tool.render(asm["k_entropy_m_lines"]))
    if int(_kernel_metadata(asm["k_entropy_m_lines"], "k_entropy_m")["sgpr_spill_count"]) > 0:
        assert regs_m, "the assembly does not name its spill VGPR any more: tools/ent_spills.py has to learn the compiler's new note"
    assert regs_c, "k_entropy_c names no spill VGPR: nothing to compare with"
    for region in PER_BIN_REGIONS:
        c = tab_m[region]
        assert c["insts"] > 0, "no instruction is attributed to '%s': the line tables or the region markers are off" % region
        assert c["spills"] == 0 and c["reloads"] == 0, "k_entropy_m: %d spills / %d reloads of scalar registers inside '%s'" % (c["spills"], c["reloads"], region)
    total_c = total_m = 0
    for region in tab_c:
        n_c, n_m = tab_c[region]["spills"] + tab_c[region]["reloads"], tab_m[region]["spills"] + tab_m[region]["reloads"]
        total_c, total_m = total_c + n_c, total_m + n_m
        if region == tool.NO_LINE:
            # not a region of the source: the instructions the compiler gives no line (here the two exits of the macroblock loop, once per slice).  Where
            # its block layout puts a reload is not the source's doing -- k_entropy_m reloads the `lane 0` mask there, 4 instructions, which k_entropy_c
            # reloads under the line that uses it; measured 5 against 1 (profiles/ent_main.txt) -- so they count in the total, not region by region;
            # but nothing may be SPILLED there
            assert tab_m[region]["spills"] == 0, "k_entropy_m spills %d scalar registers in code without a source line" % tab_m[region]["spills"]
            continue
        assert n_m <= n_c, "region '%s': k_entropy_m has %d spill / reload instructions, k_entropy_c %d" % (region, n_m, n_c)
    assert total_m < total_c, "k_entropy_m: %d spill / reload instructions in all, k_entropy_c %d" % (total_m, total_c)


def test_entropy_kernel_choice_with_the_main_kernel(H):
    lib = H.load_hooks()
    I32 = ctypes.c_int32
    f4 = lib.h264mi_internal_entropy_kernel_choice4
    f4.restype, f4.argtypes = I32, [I32, I32, I32, I32]
    GENERAL, FMO, CABAC, MAIN = 0, 1, 2, 3
    assert f4(30, 0, 0, 0) == MAIN and f4(1, 0, 0, 0) == MAIN            # all CABAC, no 8x8, no monochrome picture
    assert f4(30, 0, 0, 1) == CABAC and f4(7680, 0, 0, 7680) == CABAC    # one picture with the 8x8 transform or monochrome among them
    assert f4(255, 1, 0, 0) == GENERAL and f4(255, 1, 0, 3) == GENERAL   # one CAVLC slice
    assert f4(0, 7, 0, 0) == GENERAL
    for n_cabac, n_cavlc, n_t8 in ((5, 0, 0), (5, 0, 2), (0, 5, 0), (3, 2, 1), (0, 0, 0)):  # slice groups, whatever the rest
        assert f4(n_cabac, n_cavlc, 1, n_t8) == FMO
    assert f4(0, 0, 0, 0) in (GENERAL, FMO, CABAC, MAIN)                 # an empty level 0 (B slices only): nothing is launched, any id
    # the three-argument entry answers as before there was a Main kernel
    f3 = lib.h264mi_internal_entropy_kernel_choice
    f3.restype, f3.argtypes = I32, [I32, I32, I32]
    assert f3(30, 0, 0) == CABAC and f3(1, 0, 0) == CABAC
    assert f3(255, 1, 0) == GENERAL and f3(1, 1, 0) == GENERAL and f3(0, 7, 0) == GENERAL
    for n_cabac, n_cavlc in ((5, 0), (0, 5), (3, 2), (0, 0)):
        assert f3(n_cabac, n_cavlc, 1) == FMO
