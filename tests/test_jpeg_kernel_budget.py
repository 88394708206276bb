"""Register budget of the JPEG kernels (CPU only: hipcc cross-compiles for gfx950), in the style of test_stats_kernel_budget.py.

k_jpeg.hip has three entry points: k_jpeg_size and k_jpeg_write -- the same interval walk, counting and storing -- and k_jpeg_scan, the prefix sum of an
item's interval lengths.  A one-wavefront workgroup keeps its rows of the DCT matrix, its quantisers and the interval's state in registers; the bit buffer,
the Huffman codes and the two transposes of a block are in LDS: the 3456 bytes k_jpeg.hip states (JPEG_LDS_BYTES).  This test reads the AMDGPU metadata of
`hipcc -S` and asserts no scratch, no VGPR spill and at most 128 VGPRs.  When written the walk had 53 (size) and 57 (write) VGPRs, no AGPRs, and the write
kernel 35 SGPR spills -- uniform state of the interval, which goes to lanes of a VGPR, not to memory.  It looks at the metadata only, never at the
instructions."""
import os
import re
import shutil
import subprocess

import pytest

from test_entropy_kernel_budget import _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264decode_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the compile flags of csrc/Makefile, device side only, to assembly
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
BUDGET = {"k_jpeg_size": (128, 0, 48), "k_jpeg_write": (128, 0, 48), "k_jpeg_scan": (128, 0, 0)}  # kernel: (vgpr_count, agpr_count, sgpr_spill_count)
WALKS = ("k_jpeg_size", "k_jpeg_write")


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the build needs it too")
    out = tmp_path_factory.mktemp("jpeg_budget") / "k_jpeg.s"
    p = subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "k_jpeg.hip"), "-o", str(out)], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, "k_jpeg does not compile:\n%s" % p.stdout.decode(errors="replace")[-2000:]
    return _kernel_metadata(open(out).read())


def _stated_lds_bytes():
    src = open(os.path.join(CSRC, "k_jpeg.hip")).read()
    m = re.search(r"#define JPEG_LDS_BYTES \((.*?)\) /\*.*?: (\d+) \*/", src)
    words = int(re.search(r"#define MI_JPEG_BUF_WORDS (\d+)", open(os.path.join(CSRC, "mi_kernels.h")).read()).group(1))
    assert m and eval(m.group(1), {"MI_JPEG_BUF_WORDS": words}) == int(m.group(2)), "the file's own sum"
    return int(m.group(2))


def test_the_budget_names_every_kernel_of_the_file(metadata):
    assert sorted(metadata) == sorted(BUDGET)


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_jpeg_kernel_has_no_scratch(metadata, kernel):
    md = metadata[kernel]
    assert int(md["private_segment_fixed_size"]) == 0, "%s uses scratch: %s" % (kernel, md)
    assert int(md.get("vgpr_spill_count", 0)) == 0, md


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_jpeg_kernel_registers_and_lds_within_the_budget(metadata, kernel):
    md = metadata[kernel]
    vgprs, agprs, sgpr_spills = BUDGET[kernel]
    assert int(md["vgpr_count"]) <= vgprs, "%s: %s" % (kernel, md)
    assert int(md["vgpr_count"]) + int(md.get("agpr_count", 0)) <= vgprs + agprs, "%s: %s" % (kernel, md)
    assert int(md.get("sgpr_spill_count", 0)) <= sgpr_spills, "%s: %s" % (kernel, md)
    assert int(md["group_segment_fixed_size"]) == (_stated_lds_bytes() if kernel in WALKS else 0), "%s: %s" % (kernel, md)
