"""Resource budget of the two dbprep kernels (CPU only: hipcc cross-compiles for gfx950).

k_dbprep and k_dbprep_ip are short, memory-bound kernels that live on the number of wavefronts in flight.  A rewrite that needs more registers or
more LDS does not fail to build: the compiler spills to scratch, or fewer workgroups fit a CU.  This test reads the AMDGPU metadata of `hipcc -S`
(as test_entropy_kernel_budget.py does) and asserts, per kernel: no scratch, no spills, no dynamic stack; at most 128 registers (four wavefronts
per SIMD); at most 64 KB of static LDS per 256 threads (two 256-thread workgroups, or eight single-wavefront ones, per CU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264decode_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the compile flags of csrc/Makefile, device side only, to assembly
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
KERNELS = ("k_dbprep", "k_dbprep_ip")


def _kernel_metadata(asm):
    """The kernel-level keys of every entry of amdhsa.kernels (the .args lists sit deeper and are skipped)."""
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
    return out


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found: the build needs it too")
    tmp = tmp_path_factory.mktemp("dbprep_budget")
    p = subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, "k_dbprep.hip"), "-o", str(tmp / "k_dbprep.s")], cwd=CSRC, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT)
    assert p.returncode == 0, "k_dbprep.hip does not compile:\n%s" % p.stdout.decode(errors="replace")[-2000:]
    meta = _kernel_metadata(open(tmp / "k_dbprep.s").read())
    for k in KERNELS:
        assert k in meta, "k_dbprep.hip defines no kernel %s" % k
    return meta


@pytest.mark.parametrize("kernel", KERNELS)
def test_dbprep_kernel_has_no_scratch(metadata, kernel):
    md = metadata[kernel]
    assert int(md["private_segment_fixed_size"]) == 0, "%s spills to scratch: %s" % (kernel, md)
    assert int(md.get("vgpr_spill_count", 0)) == 0, md
    assert md.get("uses_dynamic_stack", "false") == "false", md


@pytest.mark.parametrize("kernel", KERNELS)
def test_dbprep_kernel_registers_allow_four_waves(metadata, kernel):
    md = metadata[kernel]
    regs = int(md["vgpr_count"]) + int(md.get("agpr_count", 0))
    print("%s: %d registers" % (kernel, regs))
    assert regs <= 128, "%s: %d registers (VGPR + AGPR): fewer than four wavefronts per SIMD" % (kernel, regs)


@pytest.mark.parametrize("kernel", KERNELS)
def test_dbprep_kernel_lds_allows_two_workgroups(metadata, kernel):
    md = metadata[kernel]
    threads = int(md["max_flat_workgroup_size"])
    assert threads in (64, 256), md
    lds = int(md["group_segment_fixed_size"]) * (256 // threads)  # k_dbprep_ip's workgroups are single wavefronts: four of them make 256 threads
    print("%s: %d bytes of static LDS per 256 threads" % (kernel, lds))
    assert lds <= 64 * 1024, "%s: %d bytes of static LDS per 256 threads: fewer than two such groups per CU" % (kernel, lds)
