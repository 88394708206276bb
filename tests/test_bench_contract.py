"""The bench line's contract (driver prompt, "Measurement"): the newest committed line under profiles/ carries every key the driver and
the judge read, with consistent arithmetic -- checked on the CPU, so that a refactoring of bench.py cannot silently drop one."""
import glob
import json
import os
import re

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _latest():
    files = [f for f in glob.glob(os.path.join(ROOT, "profiles", "r*_bench.json")) if re.match(r"r\d+[a-z]?_bench\.json$", os.path.basename(f))]
    assert files, "no bench line committed under profiles/"
    return max(files, key=lambda f: re.match(r"r(\d+)([a-z]?)_bench", os.path.basename(f)).groups())


def test_committed_bench_line_follows_the_contract():
    d = json.load(open(_latest()))
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == base.get("unit", d["unit"]) and d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "u8"
    assert d["vs_baseline"] is None  # BASELINE.md holds no published number for this metric
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    # achieved = algorithmic bytes per launch / launch duration (both in the line)
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["launch_ms"] * 1e-3) / 1e9) / r["achieved"] < 1e-3
    assert r["traffic"] is None or r["traffic"] >= r["algorithmic_bytes_per_launch"]  # counters cannot show less than the algorithm needs
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0
    # value is frames of the whole job over the step time
    frames = d["config"]["frames_per_step_per_gpu"] * d["n_gpus"]
    assert abs(d["value"] - frames / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.02
    assert "bit-exact" in d["parity"]


def test_bench_defaults_finish_in_minutes_by_construction():
    """bench.py with no flags: N = 1 and small K / W (the driver's default invocation)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    m = {k: int(v) for k, v in re.findall(r'add_argument\("--(gpus|steps|warmup)", type=int, default=(\d+)', src)}
    assert m["gpus"] == 1 and 1 <= m["steps"] <= 20 and m["warmup"] <= 5


def test_eight_rank_input_generation_fits_the_time_limit():
    """N > 1: every rank generates its inputs on the same host.  The plan -- distinct streams per rank x measured core-seconds per stream /
    the rank's share of the cores -- must stay far below the driver's 600 s limit on any plausible 8-GPU host, and the dry run reports it."""
    import subprocess
    import sys
    sys.path.insert(0, ROOT)
    import bench
    for cores in (64, 96, 128, 192, 256):
        assert bench.planned_generation_seconds(32, 8, cores=cores) <= 150, cores  # 8 ranks x 32 distinct 1080p GOPs
    assert bench.planned_generation_seconds(256, 1, cores=64) <= 160               # N = 1: all 256 distinct (round 3: 121 s measured)
    assert bench.generation_threads(32, 8) <= max(1, (os.cpu_count() or 8) // 8)   # a rank never takes more than its share of the host
    env = dict(os.environ, H264MI_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 8 and d["ranks_seen"] == 8 and d["distinct_streams_per_rank"] == 32
    assert d["generator_threads_per_rank"] == bench.generation_threads(32, 8)


def test_plain_run_generates_few_distinct_streams_and_full_all_of_them():
    """A plain run's setup is short: 32 distinct 1080p streams per GPU (each used 8 times), not the 256 that --full generates on one GPU."""
    import subprocess
    import sys
    for extra, want in (([], 32), (["--full"], 256)):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-run"] + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert d["n_gpus"] == 1 and d["distinct_streams_per_rank"] == want, (extra, d)


@pytest.mark.gpu
def test_gpu_plain_run_dumps_what_its_last_step_decoded(tmp_path, oracle_mod, sg):
    """bench.py --dump-outputs DIR: float32 / float64 arrays under 64 MB, the same from run to run, and the whole frames among them are the
    oracle's decode of the generated streams (stream 0 frame 0, the last stream's last frame).  The line says how many steps it timed."""
    import subprocess
    import sys
    import numpy as np
    S, F, W, Hh = 8, 4, 320, 240
    dumps = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--streams", str(S), "--frames", str(F),
               "--width", str(W), "--height", str(Hh), "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=ROOT, env=dict(os.environ, H264MI_BENCH_CACHE="off"))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["unit"] == "frames/s" and line["higher_is_better"] is True
        assert abs(line["value"] - S * F / (line["ms_per_step"] * 1e-3)) / line["value"] < 0.02
        files = sorted(os.listdir(d))
        assert files and sum(os.path.getsize(os.path.join(d, f)) for f in files) <= 64e6
        arrs = {f: np.load(os.path.join(d, f), allow_pickle=False) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        dumps.append(arrs)
    assert dumps[0].keys() == dumps[1].keys() and all(np.array_equal(dumps[0][f], dumps[1][f]) for f in dumps[0])
    a = dumps[0]
    assert (a["stream_status.npy"] == 0).all() and a["stream_status.npy"].shape == (S,)
    assert a["frame_index.npy"].tolist() == [[0, 0], [S - 1, F - 1]]
    for (s, f), got in zip(a["frame_index.npy"].astype(int), a["frames.npy"]):
        stream = sg.encode(**sg.recipe("C3", frames=F, idr_period=F, seed=1000 + s, width=W, height=Hh))[0]
        ref, _ = oracle_mod.decode(stream, crop=True)
        assert np.array_equal(got, ref[f].astype(np.float32)), (s, f)
