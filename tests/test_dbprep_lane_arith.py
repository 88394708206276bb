"""The per-lane arithmetic of k_dbprep_ip (ip_dbprm in k_dbprep.hip: bit-parallel "coefficients" masks, packed 16-bit vector compare, the
parameter packing) against k_dbprep's rules, on the CPU: tools/dbprep_lane_check.hip compiles the function as host code and runs it over
random macroblock records, including near-identical neighbours, vectors at the ends of the 16-bit range and garbage records.  Every byte of
every DbPrm must agree -- no tolerance.  (What the kernel does around that function -- loads, neighbours, stores, the intra mask -- is the GPU
tests' business: tests/test_dbprep_lanes.py.)"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_lane_arithmetic_matches_k_dbprep_on_random_records(tmp_path):
    exe = str(tmp_path / "dbprep_lane_check")
    p = subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "h264decode_amd", "csrc"), "-x", "hip",
                        os.path.join(ROOT, "tools", "dbprep_lane_check.hip"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0, "tools/dbprep_lane_check.hip does not compile:\n%s" % p.stdout.decode(errors="replace")[-2000:]
    r = subprocess.run([exe, "400000"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = r.stdout.decode(errors="replace")
    print(out[-2000:])
    assert r.returncode == 0 and "400000 cases, 0 mismatches" in out
