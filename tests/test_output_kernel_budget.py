"""Register budget of the output kernels K7 .. K9 (CPU only: hipcc cross-compiles for gfx950).

k_convert.hip, k_scale.hip and k_tensor.hip share one copy of the conversion and sampling rule (k_output_rule.h).  Everything in that header is
inlined, so each kernel keeps a register allocation of its own -- but a change of the shared text moves all five kernels at once, and a kernel
that needs more registers does not fail to build: it loses waves per SIMD or spills.  This test reads the AMDGPU metadata of `hipcc -S` and
asserts, per kernel, no scratch and no VGPR spill at all, and no more registers and SGPR spills than the kernels had while each carried its own
copy of the rule (the register table of profiles/output_refactor.txt).  It looks at the metadata only, never at the instructions."""
import os
import shutil
import subprocess

import pytest

from test_entropy_kernel_budget import _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264decode_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the compile flags of csrc/Makefile, device side only, to assembly
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
SOURCES = ("k_convert", "k_scale", "k_tensor")
# kernel: (vgpr_count, agpr_count, sgpr_spill_count) with a private copy of the rule in every file.  vgpr_count is the whole unified allocation, the
# AGPRs included (k_scale: 256 + 160)
BUDGET = {"k_convert": (150, 0, 0), "k_scale": (416, 160, 26), "k_scale_area": (197, 0, 2), "k_tensor": (131, 0, 321), "k_tensor_area": (125, 0, 141)}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the build needs it too")
    tmp = tmp_path_factory.mktemp("out_budget")
    procs = {}
    for k in SOURCES:  # the three compiles side by side
        procs[k] = subprocess.Popen([HIPCC] + FLAGS + [os.path.join(CSRC, k + ".hip"), "-o", str(tmp / (k + ".s"))], cwd=CSRC,
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    meta = {}
    for k, p in procs.items():
        log = p.communicate()[0].decode(errors="replace")
        assert p.returncode == 0, "%s does not compile:\n%s" % (k, log[-2000:])
        meta.update(_kernel_metadata(open(tmp / (k + ".s")).read()))
    return meta


def test_the_budget_names_every_output_kernel(metadata):
    assert sorted(metadata) == sorted(BUDGET)


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_output_kernel_has_no_scratch(metadata, kernel):
    md = metadata[kernel]
    assert int(md["private_segment_fixed_size"]) == 0, "%s uses scratch: %s" % (kernel, md)
    assert int(md.get("vgpr_spill_count", 0)) == 0, md


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_output_kernel_registers_within_the_budget(metadata, kernel):
    md = metadata[kernel]
    vgprs, agprs, sgpr_spills = BUDGET[kernel]
    assert int(md["vgpr_count"]) <= vgprs, "%s: %s" % (kernel, md)
    assert int(md["vgpr_count"]) + int(md.get("agpr_count", 0)) <= vgprs + agprs, "%s: %s" % (kernel, md)
    assert int(md.get("sgpr_spill_count", 0)) <= sgpr_spills, "%s: %s" % (kernel, md)
