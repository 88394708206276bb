"""The budgets of p16_fast, the P_L0_16x16 path of k_entropy_c and k_entropy_m (k_entropy.hip under MI_ENT_P16), on the CPU: hipcc cross-compiles
for gfx950, tools/ent_spills.py attributes instructions and scalar spill traffic to the `// @region` lines of the source.  Both kernels keep
the register budget (no scratch, no spilled VGPR, at most 80 VGPRs: six waves per SIMD) and do not spill more scalar registers than the kernels
had before the path existed (33 and 27); p16_fast itself and the code that runs per bin and per residual block are free of spill traffic;
either kernel is smaller than k_entropy of the same tree; pskip_fast, which shares the vector prediction and the write-out with the new path,
has not grown.  (The pictures are in test_entropy_p16_gpu.py; the measurements in profiles/ent_p16.txt.)"""
import os
import subprocess

import pytest

from test_entropy_main_kernel import CSRC, FLAGS, HIPCC, _kernel_metadata, _tool

KERNELS = ("k_entropy_c", "k_entropy_m")
SPILLED_SGPRS_BEFORE = {"k_entropy_c": 33, "k_entropy_m": 27}
PSKIP_INSTS_BEFORE = 152  # instructions of the pskip_fast region in either kernel before it shared its halves
CLEAN_REGIONS = ("p16_fast", "bit reader", "CABAC engine", "cabac_residual", "parse_residual_cabac")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    """k_entropy_c and k_entropy_m with the budget flags and once more with line tables, and k_entropy for its size: five compiles side by side"""
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the build needs it too")
    tmp = tmp_path_factory.mktemp("ent_p16")
    jobs = {"k_entropy": ("k_entropy", [])}
    for k in KERNELS:
        jobs[k] = (k, [])
        jobs[k + "_lines"] = (k, ["-gline-tables-only"])
    procs = {key: subprocess.Popen([HIPCC] + FLAGS + extra + [os.path.join(CSRC, src + ".hip"), "-o", str(tmp / (key + ".s"))], cwd=CSRC,
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for key, (src, extra) in jobs.items()}
    out = {}
    for key, p in procs.items():
        log = p.communicate()[0].decode(errors="replace")
        assert p.returncode == 0, "%s does not compile:\n%s" % (key, log[-2000:])
        out[key] = open(tmp / (key + ".s")).read()
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_p16_kernels_keep_the_register_budget(kernel, asm):
    md = _kernel_metadata(asm[kernel], kernel)
    print("%s: %s VGPRs, %s spilled SGPRs, %d code bytes" % (kernel, md["vgpr_count"], md["sgpr_spill_count"], md["code_len"]))
    assert int(md["private_segment_fixed_size"]) == 0, "%s spills to scratch: %s" % (kernel, md)
    assert int(md.get("vgpr_spill_count", 0)) == 0 and md.get("uses_dynamic_stack", "false") == "false", md
    assert int(md["vgpr_count"]) + int(md.get("agpr_count", 0)) <= 80, md
    assert int(md["sgpr_spill_count"]) <= SPILLED_SGPRS_BEFORE[kernel], md


@pytest.mark.parametrize("kernel", KERNELS)
def test_p16_kernels_are_smaller_than_the_general_one(kernel, asm):
    own, general = _kernel_metadata(asm[kernel], kernel)["code_len"], _kernel_metadata(asm["k_entropy"], "k_entropy")["code_len"]
    print("code bytes: %s %d, k_entropy %d" % (kernel, own, general))
    assert own < general


@pytest.mark.parametrize("kernel", KERNELS)
def test_p16_region_and_per_bin_code_without_spill_traffic(kernel, asm):
    tool = _tool()
    assert "p16_fast" in [name for _, name in tool.regions()], "k_entropy.hip has lost its `// @region p16_fast` line"
    tab, regs, _ = tool.table(asm[kernel + "_lines"])
    print(kernel + "\n" + tool.render(asm[kernel + "_lines"]))
    if int(_kernel_metadata(asm[kernel + "_lines"], kernel)["sgpr_spill_count"]) > 0:
        assert regs, "the assembly does not name its spill VGPR any more: tools/ent_spills.py has to learn the compiler's new note"
    for region in CLEAN_REGIONS:
        c = tab[region]
        assert c["insts"] > 0, "no instruction is attributed to '%s': the line tables or the region markers are off" % region
        assert c["spills"] == 0 and c["reloads"] == 0, "%s: %d spills / %d reloads of scalar registers inside '%s'" % (kernel, c["spills"], c["reloads"], region)
    assert 0 < tab["pskip_fast"]["insts"] <= PSKIP_INSTS_BEFORE, tab["pskip_fast"]
