"""Resource budget of the reconstruction kernels: K3 (k_intra, k_intra_x), K4 (k_inter, k_inter_b), K5 (k_deblock, k_deblock_x) and k_conceal
(CPU only: hipcc cross-compiles for gfx950).

These kernels share their helpers (k_common.h, k_residual.h) and, in K3, one macroblock step between two schedulers.  A change to a shared piece
that costs registers does not fail to build: the compiler spills to scratch or fewer wavefronts fit a SIMD -- and k_deblock issues loads into
registers behind the compiler's back (ALD16M / ALD_PHASE), which is only sound while none of them is spilled or copied.  This test reads the AMDGPU
metadata of `hipcc -S` with the flags of csrc/Makefile (as test_dbprep_kernel_budget.py does) and asserts, per kernel: no scratch, no spilled
vector register, no dynamic stack, and no more vector registers than the kernel had when the helpers were folded (measured then with the same
flags; a kernel that gets by with fewer may lower its line).  Metadata only: no instruction text is looked at."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "h264decode_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the compile flags of csrc/Makefile, device side only, to assembly
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "--offload-arch=gfx950", "--cuda-device-only", "-S"]
# kernel -> (source file, VGPRs + AGPRs it may use)
KERNELS = {
    "k_intra": ("k_recon", 99),
    "k_intra_x": ("k_recon", 115),
    "k_inter": ("k_inter", 85),
    "k_inter_b": ("k_inter", 90),
    "k_deblock": ("k_deblock", 228),
    "k_deblock_x": ("k_deblock_x", 96),
    "k_conceal": ("k_conceal", 36),
}


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
    tmp = tmp_path_factory.mktemp("recon_budget")
    sources = sorted({src for src, _ in KERNELS.values()})
    procs = {}
    for src in sources:  # the five files compile side by side
        procs[src] = subprocess.Popen([HIPCC] + FLAGS + [os.path.join(CSRC, src + ".hip"), "-o", str(tmp / (src + ".s"))], cwd=CSRC,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    meta = {}
    for src, p in procs.items():
        out = p.communicate()[0]
        assert p.returncode == 0, "%s.hip does not compile:\n%s" % (src, out.decode(errors="replace")[-2000:])
        meta[src] = _kernel_metadata(open(tmp / (src + ".s")).read())
    for k, (src, _) in KERNELS.items():
        assert k in meta[src], "%s.hip defines no kernel %s" % (src, k)
    return {k: meta[src][k] for k, (src, _) in KERNELS.items()}


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_recon_kernel_has_no_scratch(metadata, kernel):
    md = metadata[kernel]
    assert int(md["private_segment_fixed_size"]) == 0, "%s spills to scratch: %s" % (kernel, md)
    assert int(md.get("vgpr_spill_count", 0)) == 0, md
    assert md.get("uses_dynamic_stack", "false") == "false", md


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_recon_kernel_registers_within_budget(metadata, kernel):
    md = metadata[kernel]
    regs = int(md["vgpr_count"]) + int(md.get("agpr_count", 0))
    limit = KERNELS[kernel][1]
    print("%s: %d registers (limit %d), %s SGPRs, %s bytes of static LDS, %s spilled SGPRs" %
          (kernel, regs, limit, md.get("sgpr_count"), md.get("group_segment_fixed_size"), md.get("sgpr_spill_count", 0)))
    assert regs <= limit, "%s: %d registers (VGPR + AGPR), it had %d" % (kernel, regs, limit)
