"""The stand-alone programs of tools/ that drive the product's host side against the null device of tools/hoststub (host_pocs.sh,
host_dpb_trace.sh: g++, no GPU): built for the test modules that run them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(script, tmp):
    """Runs tools/<script> with its output under `tmp`; the path of the program it built."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", script)], env=dict(os.environ, TMPDIR=str(tmp)), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().splitlines()[-1]
