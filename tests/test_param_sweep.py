"""A fixed slice of tools/param_sweep.py in the suite: random recipes over the generator's whole feature space, decoder output against the
generator's reconstruction bit for bit.  (The open-ended hunt is the tool itself; the seeds here are the ones that found nothing after the
round-3 fixes, so a failure is a regression.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
TOOL = os.path.join(ROOT, "tools", "param_sweep.py")


def _sweep(*args):
    r = subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and "0 mismatches" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_sweep_oracle_equals_generator():
    _sweep("400", "--seed", "3")
    _sweep("150", "--seed", "5", "--concat")
    _sweep("300", "--seed", "61", "--extreme")
    _sweep("400", "--seed", "21", "--fields")  # field pictures (PAFF)
    _sweep("300", "--seed", "71", "--ranges")  # weights, picture order count distances, vectors, 0 / 255 content and scaling lists at the ends of their ranges
    _sweep("150", "--seed", "72", "--ranges", "--fields")


@pytest.mark.gpu
@pytest.mark.parametrize("args", [("300", "--seed", "11"), ("200", "--seed", "31", "--split"), ("40", "--seed", "23", "--batch", "6"),
                                  ("150", "--seed", "5", "--concat"), ("150", "--seed", "13", "--concat", "--split"), ("40", "--seed", "9", "--big"),
                                  ("250", "--seed", "41", "--xwgs"), ("300", "--seed", "61", "--extreme"),
                                  ("250", "--seed", "21", "--fields"), ("200", "--seed", "22", "--fields", "--split"), ("100", "--seed", "23", "--fields", "--xwgs"),
                                  ("60", "--seed", "24", "--fields", "--big"),
                                  ("300", "--seed", "71", "--ranges"), ("150", "--seed", "72", "--ranges", "--fields"), ("150", "--seed", "73", "--ranges", "--split")])
def test_gpu_sweep_equals_generator(args):
    _sweep(*args, "--gpu")
