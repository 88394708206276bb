"""Register budget of the three entropy kernels (CPU only: hipcc cross-compiles for gfx950).

The entropy kernels are long-lived, one wavefront per slice, and share the chip with the reconstruction kernels of the previous
pass, so each is built for a fixed number of waves per SIMD (k_entropy.hip: MI_ENT_MINWAVES).  A rewrite that needs more registers
than that budget does not fail to build: the compiler silently spills to scratch.  This test reads the AMDGPU metadata of
`hipcc -S` and asserts, per kernel, no scratch at all and a VGPR count that still allows the intended number of waves."""
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
KERNELS = ("k_entropy", "k_entropy_b", "k_entropy_f")


def _min_waves(kernel):
    """Waves per SIMD the kernel is built for: its own MI_ENT_MINWAVES (else k_entropy.hip's default); the B kernel names its budget in
    its amdgpu_waves_per_eu attribute."""
    common = open(os.path.join(CSRC, "k_entropy.hip")).read()
    if kernel == "k_entropy_b":
        return int(re.search(r"amdgpu_waves_per_eu\((\d+),\s*\d+\)\)\)\s*k_entropy_b\b", common).group(1))
    own = re.search(r"^#define MI_ENT_MINWAVES (\d+)", open(os.path.join(CSRC, kernel + ".hip")).read(), re.M)
    return int(own.group(1)) if own else int(re.search(r"#ifndef MI_ENT_MINWAVES\s+#define MI_ENT_MINWAVES (\d+)", common).group(1))


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
    tmp = tmp_path_factory.mktemp("ent_budget")
    procs = {}
    for k in KERNELS:  # the three compiles side by side
        procs[k] = subprocess.Popen([HIPCC] + FLAGS + [os.path.join(CSRC, k + ".hip"), "-o", str(tmp / (k + ".s"))], cwd=CSRC,
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    meta = {}
    for k, p in procs.items():
        log = p.communicate()[0].decode(errors="replace")
        assert p.returncode == 0, "%s does not compile:\n%s" % (k, log[-2000:])
        meta.update(_kernel_metadata(open(tmp / (k + ".s")).read()))
    return meta


@pytest.mark.parametrize("kernel", KERNELS)
def test_entropy_kernel_has_no_scratch(metadata, kernel):
    md = metadata[kernel]
    assert int(md["private_segment_fixed_size"]) == 0, "%s spills to scratch: %s" % (kernel, md)
    assert int(md.get("vgpr_spill_count", 0)) == 0, md
    assert md.get("uses_dynamic_stack", "false") == "false", md


@pytest.mark.parametrize("kernel", KERNELS)
def test_entropy_kernel_vgprs_allow_its_waves(metadata, kernel):
    md = metadata[kernel]
    # gfx950: 512 registers per lane and SIMD, shared by the VGPRs and AGPRs of the resident waves, allocated in granules of 8
    regs = int(md["vgpr_count"]) + int(md.get("agpr_count", 0))
    waves = min(8, 512 // (-(-regs // 8) * 8))
    assert waves >= _min_waves(kernel), "%s: %d registers allow %d waves per SIMD, built for %d" % (kernel, regs, waves, _min_waves(kernel))
