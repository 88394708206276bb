"""Register budget of the frame statistics kernel (CPU only: hipcc cross-compiles for gfx950), in the style of test_deint_motion_kernel_budget.py.

k_stats.hip is the project's one reduction: eight instantiations of one thread item (aligned or byte path x with or without a predecessor x luma or
chroma) behind one entry point, a 256-bin histogram per wavefront in LDS, and the cross-lane sums.  This test reads the AMDGPU metadata of `hipcc -S` and
asserts no scratch, no VGPR spill, and at most 128 VGPRs: four waves per SIMD, which the kernel also asks for (__launch_bounds__(256, 4)).  When written
the kernel had 58 VGPRs, no AGPRs, 4096 bytes of LDS (four wavefronts x 256 bins x 4 bytes: the histogram variant the kernel was measured and shipped
with) and 11 SGPR spills -- the uniform state of the eight instantiations; they go to lanes of a VGPR, not to memory.  It looks at the metadata only, never
at the instructions."""
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
BUDGET = {"k_stats": (128, 0, 16)}  # kernel: (vgpr_count, agpr_count, sgpr_spill_count)
LDS_BYTES = 4096


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the build needs it too")
    out = tmp_path_factory.mktemp("stats_budget") / "k_stats.s"
    p = subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "k_stats.hip"), "-o", str(out)], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, "k_stats does not compile:\n%s" % p.stdout.decode(errors="replace")[-2000:]
    return _kernel_metadata(open(out).read())


def test_the_budget_names_every_kernel_of_the_file(metadata):
    assert sorted(metadata) == sorted(BUDGET)


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_stats_kernel_has_no_scratch(metadata, kernel):
    md = metadata[kernel]
    assert int(md["private_segment_fixed_size"]) == 0, "%s uses scratch: %s" % (kernel, md)
    assert int(md.get("vgpr_spill_count", 0)) == 0, md


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_stats_kernel_registers_and_lds_within_the_budget(metadata, kernel):
    md = metadata[kernel]
    vgprs, agprs, sgpr_spills = BUDGET[kernel]
    assert int(md["vgpr_count"]) <= vgprs, "%s: %s" % (kernel, md)
    assert int(md["vgpr_count"]) + int(md.get("agpr_count", 0)) <= vgprs + agprs, "%s: %s" % (kernel, md)
    assert int(md.get("sgpr_spill_count", 0)) <= sgpr_spills, "%s: %s" % (kernel, md)
    assert int(md["group_segment_fixed_size"]) == LDS_BYTES, "%s: %s" % (kernel, md)
