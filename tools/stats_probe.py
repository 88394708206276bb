"""K12 (k_stats) next to K6 (k_pack) over the same frames, and next to the torch route it replaces.

    python tools/stats_probe.py [--streams 64] [--distinct 32] [--frames 30] [--reps 21] [--torch-frames 128]

One process, the bench's clean 1080p batch (bench.gen_stream: the same generator recipe and seeds), as tools/deint_probe.py.  Every figure is the median
of --reps launches, wall clock around launch + synchronise of the decoder's stream, as ms, as GB/s of the ALGORITHMIC bytes per pixel -- 1.5 read for a
record, 3.0 with a predecessor; K6 reads 1.5 and writes 1.5 -- and as a ratio to K6's time in the same run.  Four configurations, the item array built
once, outside the timing:
    record only            no predecessor, no grid
    predecessor            every frame against frame f - 1 of its stream (frame 0: frame 1)
    predecessor + grid     the same with both planes of cell size 16
    flat, record only      the contention case of the histogram: the luma of every frame of the pool overwritten with one value (a torch fill through
                           h264mi_frame_device_planes), measured LAST; "flat, predecessor" likewise
The torch route, for comparison, over the first --torch-frames frames (its intermediates are 8 bytes a sample) and scaled to all of them: K6 into a
tensor, then per frame a bincount of the luma, its sum, and the sum of absolute differences against the frame before through int16.
Before timing, the records of the first launch are held to torch: sum_y, the histogram and sad_y of the first frames.
H264MI_LIB=<a build with -DMI_STATS_HIST=0 / 1 / 2> compares the kernel's three answers to histogram contention (csrc/k_stats.hip)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import h264decode_amd as H  # noqa: E402
from h264decode_amd import _lib  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--torch-frames", type=int, default=128)
    ap.add_argument("--label", default="", help="a word for the summary line: which build this is")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    S, F, w, h = args.streams, args.frames, args.width, args.height
    nd = max(1, min(args.distinct, S))
    with ThreadPoolExecutor(max_workers=min(16, nd)) as ex:
        gen = list(ex.map(bench.gen_stream, [(1000 + i, F, w, h) for i in range(nd)]))
    streams = [gen[i % nd][0] for i in range(S)]
    W, Hc = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    dec = H.Decoder(max_streams=S, max_width=W, max_height=Hc, max_frames_per_batch=F, max_slices_per_frame=1,
                    max_bitstream_bytes=int(sum(len(s) for s in streams) * 1.1) + (1 << 20), hip_stream=torch.cuda.current_stream().cuda_stream)
    dec.decode(streams)
    n, px = S * F, w * h
    i420 = torch.empty((n, px * 3 // 2), dtype=torch.uint8, device="cuda")
    one_rec, one_grid = dec.stats_size(w, h)[2], dec.stats_size(w, h, 16, 3)[2]
    out = torch.empty(n * one_grid // 8, dtype=torch.int64, device="cuda")

    def items(prev):
        arr = (_lib.StatsItem * n)()
        for i, a in enumerate(arr):
            a.stream, a.frame = i // F, i % F
            a.prev_frame = H.STATS_PREV_NONE if not prev else (a.frame - 1 if a.frame else min(1, F - 1))
        return arr
    alone, against = items(False), items(True)

    def launch(arr, cell=0, planes=0):
        got = ctypes.c_size_t(0)
        _lib.check(dec._L.h264mi_items_stats_device(dec._h, ctypes.byref(H.stats_spec(cell, planes, 8)), arr, n, out.data_ptr(), out.numel() * 8, ctypes.byref(got)))

    def timed(fn):
        fn()
        dec.sync()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            dec.sync()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    rows = []

    def row(name, fn, bytes_per_px, frames=n):
        ms = timed(fn) * n / frames
        gbs = bytes_per_px * px * n / (ms * 1e-3) / 1e9
        rows.append({"what": name, "ms": round(ms, 3), "GB/s": round(gbs, 1), "share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3), "algorithmic_bytes_per_pixel": bytes_per_px})
        print(json.dumps(rows[-1]), flush=True)

    # the same numbers first: the first frames' records against torch on K6's frames
    dec.pack_batch(i420.data_ptr(), i420.numel())
    launch(against)
    dec.sync()
    k = min(8, n)
    rec = out[:n * one_rec // 8].view(n, one_rec // 8)
    luma = i420[:k, :px].to(torch.int64)
    assert torch.equal(rec[:k, 0], luma.sum(dim=1)), "sum_y"
    assert torch.equal(rec[:k, 4][1:], (luma[1:] - luma[:-1]).abs().sum(dim=1)), "sad_y"
    hist = rec[:k, 12:].contiguous().view(torch.int32).view(k, 256).to(torch.int64)
    assert torch.equal(hist, torch.stack([torch.bincount(luma[i], minlength=256) for i in range(k)])), "hist_y"
    del luma, hist, rec

    row("k_pack (K6) I420", lambda: dec.pack_batch(i420.data_ptr(), i420.numel()), 3.0)
    row("k_stats record only", lambda: launch(alone), 1.5)
    row("k_stats predecessor", lambda: launch(against), 3.0)
    row("k_stats predecessor + grid 16", lambda: launch(against, 16, 3), 3.0)

    tf = max(2, min(args.torch_frames, n))

    def torch_route():
        dec.pack_batch(i420.data_ptr(), i420.numel())
        dec.sync()
        y = i420[:tf, :px]
        idx = y.to(torch.int64) + 256 * torch.arange(tf, device="cuda").view(tf, 1)
        torch.bincount(idx.view(-1), minlength=256 * tf)
        y.sum(dim=1, dtype=torch.int64)
        d = y.to(torch.int16)
        (d[1:] - d[:-1]).abs().sum(dim=1, dtype=torch.int64)
    row("torch route (K6 + bincount + sums + |diff|), scaled from %d frames" % tf, torch_route, 3.0, frames=tf)

    # the contention case last: one value in every luma sample of the pool
    class Plane:  # a frame's luma plane in the pool as a torch tensor (no copy): torch takes a device pointer through this interface
        def __init__(self, ptr, nbytes):
            self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    for s in range(S):
        for f in range(F):
            y = ctypes.c_void_p()
            _lib.check(dec._L.h264mi_frame_device_planes(dec._h, s, f, ctypes.byref(y), None, None, None, None, None, None))
            torch.as_tensor(Plane(y.value, W * Hc), device="cuda").fill_(119)
    torch.cuda.synchronize()
    launch(alone)
    dec.sync()
    rec = out[:n * one_rec // 8].view(n, one_rec // 8)
    assert int(rec[0, 0]) == 119 * px and int(rec[n - 1, 0]) == 119 * px, "the flat frames"
    rec32 = out.view(torch.int32)[:n * one_rec // 4].view(n, one_rec // 4)  # min_y, max_y at words 16, 17; hist_y[v] at word 24 + v
    assert bool((rec32[:, 16] == 119).all()) and bool((rec32[:, 17] == 119).all()), "min_y, max_y of the flat frames"
    assert bool((rec32[:, 24 + 119] == px).all()) and bool((rec32[:, 24:].sum(dim=1) == px).all()), "hist_y of the flat frames: one bin"
    row("k_stats flat, record only", lambda: launch(alone), 1.5)
    row("k_stats flat, predecessor", lambda: launch(against), 3.0)
    dec.close()
    k6 = rows[0]["ms"]
    print(json.dumps({"label": args.label, "lib": os.path.basename(os.environ.get("H264MI_LIB", "libh264mi.so")), "frames": n, "size": "%dx%d" % (w, h), "reps": args.reps,
                      "time_over_k_pack": {r["what"]: round(r["ms"] / k6, 3) for r in rows[1:]}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
