"""K10 (k_deint, k_deint_motion) next to K6 (k_pack) over the same frames: one-read, one-write frame kernels, and the two-read motion-adaptive one.

    python tools/deint_probe.py [--streams 64] [--distinct 32] [--frames 30] [--reps 5]

One process, the bench's clean 1080p batch (bench.gen_stream: the same generator recipe and seeds).  Every figure is the median of --reps launches, wall
clock around launch + synchronise of the decoder's stream, as ms and as GB/s of the ALGORITHMIC bytes per pixel: 1.5 read + 1.5 written for K6 and for
BLEND; FIELD and EDGE read the kept rows only (0.75) and write 1.5; the motion-adaptive modes read the frame and its predecessor whole and write one
frame (4.5) -- their rows give EVERY frame a predecessor through the item call (frame f - 1; frame 0: frame 1), with the item array built once, outside the
timing.  "motion batch" and "motion batch+history" are the batch call without and with H264MI_DEINT_HISTORY over the same frames (the first frame of each
stream has no predecessor there, or the history): their difference is the cost of the history copies, one frame per stream.  The arena of the derived
frames is allocated by the warm-up call, outside the timing.
Before timing, FIELD's kept rows are compared with K6's frames and BLEND of a frame with itself through torch.  The expectation: FIELD and BLEND take at
most 1.25 x K6's time; EDGE is reported without a bound.  If the I420 copy of the batch and the arena do not fit beside the decoder, run with fewer --streams."""
import argparse
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

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="under a profiler: launch only the rows whose name contains this (e.g. 'field'), without the equality checks")
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

    def row(name, fn, bytes_per_px):
        if args.only in name:
            ms = timed(fn)
            gbs = bytes_per_px * px * n / (ms * 1e-3) / 1e9
            rows.append({"what": name, "ms": round(ms, 3), "GB/s": round(gbs, 1), "share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3), "algorithmic_bytes_per_pixel": bytes_per_px})

    if not args.only:
        # the same bytes first: the kept rows of FIELD are K6's rows; BLEND of rows (a, b, c) is (a + 2 b + c + 2) >> 2
        dec.pack_batch(i420.data_ptr(), i420.numel())
        assert dec.deinterlace(-1, "field", 1) == n
        got = torch.empty_like(i420)
        dec.pack_batch(got.data_ptr(), got.numel(), stream=H.STREAM_DERIVED)
        dec.sync()
        ya, yb = i420[:, :px].view(n, h, w), got[:, :px].view(n, h, w)
        assert torch.equal(ya[:, 0::2], yb[:, 0::2]), "FIELD does not keep the even rows"
        mid = (ya[:8, 0:-2:2].to(torch.int32) + ya[:8, 2::2].to(torch.int32) + 1) >> 1
        assert torch.equal(mid.to(torch.uint8), yb[:8, 1:-1:2]), "FIELD's missing rows are not the rounded mean of their neighbours"
        assert dec.deinterlace(-1, "blend", 1) == n
        dec.pack_batch(got.data_ptr(), got.numel(), stream=H.STREAM_DERIVED)
        dec.sync()
        y = ya[:8].to(torch.int32)
        assert torch.equal(((y[:, :-2] + 2 * y[:, 1:-1] + y[:, 2:] + 2) >> 2).to(torch.uint8), yb[:8, 1:-1]), "BLEND is not (a + 2 b + c + 2) >> 2"
        # motion-adaptive: a frame against itself is the frame (m = 0 everywhere)
        assert dec.deinterlace(mode="motion_edge", items=[(s, f, 0, f) for s in range(S) for f in range(F)]) == n
        dec.pack_batch(got.data_ptr(), got.numel(), stream=H.STREAM_DERIVED)
        dec.sync()
        assert torch.equal(got, i420), "motion-adaptive: a frame that is its own predecessor is not itself"
        del got, ya, yb, y, mid

    row("k_pack (K6) I420", lambda: dec.pack_batch(i420.data_ptr(), i420.numel()), 3.0)
    row("k_deint field", lambda: dec.deinterlace(-1, "field", 1), 2.25)
    row("k_deint blend", lambda: dec.deinterlace(-1, "blend", 1), 3.0)
    row("k_deint edge", lambda: dec.deinterlace(-1, "edge", 1), 2.25)
    from h264decode_amd import _lib
    arr = (_lib.DeintMotionItem * n)()
    for i, a in enumerate(arr):
        a.stream, a.frame, a.parity = i // F, i % F, 0
        a.prev_frame = a.frame - 1 if a.frame else min(1, F - 1)

    def motion_items(mode):
        _lib.check(dec._L.h264mi_items_deinterlace_motion(dec._h, mode, arr, n, None))
    row("k_deint_motion motion", lambda: motion_items(H.DEINT_FIELD), 4.5)
    row("k_deint_motion motion_edge", lambda: motion_items(H.DEINT_EDGE), 4.5)
    row("k_deint_motion motion batch", lambda: dec.deinterlace(-1, "motion", 1), 4.5)
    row("k_deint_motion motion batch+history", lambda: dec.deinterlace(-1, "motion", 1, history=True), 4.5)
    dec.close()
    for r in rows:
        print(json.dumps(r))
    if args.only:
        return 0
    k6 = rows[0]["ms"]
    ratios = {r["what"].split(" ", 1)[1]: round(r["ms"] / k6, 3) for r in rows[1:]}
    ok = ratios["field"] <= 1.25 and ratios["blend"] <= 1.25
    print(json.dumps({"frames": n, "size": "%dx%d" % (w, h), "reps": args.reps, "time_over_k_pack": ratios, "field_and_blend_within_1.25x_k_pack": ok}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
