"""K11 (k_side) next to K6 (k_pack) over the same frames, and next to the route a caller had before K11.

    python tools/side_probe.py [--streams 64] [--distinct 32] [--frames 30] [--reps 21] [--host-frames 4]

One process, two batches: the bench's clean 1080p I P P P batch (bench.gen_stream: the same generator recipe and seeds) and the same recipe as I B B P.
Every device figure is the median of --reps launches, wall clock around launch + synchronise of the decoder's stream, as ms and as GB/s of the
ALGORITHMIC bytes per macroblock: K6 reads and writes 384; K11 reads the 128-byte record (and 64 bytes of list-1 vectors in pictures with B slices when
a list-1 vector plane is selected) and writes 32 per plane.  The host route -- h264mi_frame_read_mbrecs / _mbmv1 per frame (a synchronising copy each)
plus the numpy rearrangement of tests/sideutil.py -- is timed on --host-frames frames and scaled to the batch.  Before timing, K11's planes of those
frames are compared with that rearrangement.  The expectation: all twelve planes take no longer than K6, the four list-0 motion planes no longer than
0.6 x K6.  If the buffers do not fit beside the decoder, run with fewer --streams."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import h264decode_amd as H  # noqa: E402
import sideutil  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
L0 = ("mvx0", "mvy0", "ref0", "dpoc0")


def host_route(dec, stream, frame, wmb, hmb, bits):
    """What a caller did before K11: the raw records of one frame to the host, rearranged there."""
    fi = dec.frame_info(stream, frame)
    pocs = {}
    for s in range(-1, 64):
        try:
            cur, l0 = dec.ref_pocs(stream, frame, s, 0)
        except H.H264MIError:
            break
        pocs[s] = (cur, l0, dec.ref_pocs(stream, frame, s, 1)[1])
    return sideutil.frame(dec.read_mbrecs(stream, frame, wmb * hmb), dec.read_mbmv1(stream, frame, wmb * hmb), wmb, hmb, fi.crop_x, fi.crop_y, fi.width, fi.height, pocs, bits)


def measure(label, over, args):
    S, F, w, h = args.streams, args.frames, args.width, args.height
    nd = max(1, min(args.distinct, S))
    with ThreadPoolExecutor(max_workers=min(16, nd)) as ex:
        gen = list(ex.map(bench.gen_stream, [(1000 + i, F, w, h, over) for i in range(nd)]))
    streams = [gen[i % nd][0] for i in range(S)]
    W, Hc = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    wmb, hmb = W // 16, Hc // 16
    dec = H.Decoder(max_streams=S, max_width=W, max_height=Hc, max_frames_per_batch=F, max_slices_per_frame=1,
                    max_bitstream_bytes=int(sum(len(s) for s in streams) * 1.1) + (1 << 20), hip_stream=torch.cuda.current_stream().cuda_stream)
    dec.decode(streams)
    n, mbs = S * F, wmb * hmb
    has_b = bool(over.get("bframes"))
    i420 = torch.empty((n, w * h * 3 // 2), dtype=torch.uint8, device="cuda")
    one_all, one_l0 = dec.side_size(H.SIDE_ALL, w, h)[2], dec.side_size(L0, w, h)[2]
    side = torch.empty(n * one_all, dtype=torch.uint8, device="cuda")

    # the same values first: K11's planes of a few frames against the host route
    dec.side_batch(side.data_ptr(), side.numel(), H.SIDE_ALL)
    dec.sync()
    picks = [(k * 7919) % n for k in range(args.host_frames)]
    t0 = time.perf_counter()
    wants = [host_route(dec, k // F, k % F, wmb, hmb, sideutil.ALL) for k in picks]
    host_ms = (time.perf_counter() - t0) * 1e3 / len(picks) * n
    for k, want in zip(picks, wants):
        got = side[k * one_all:(k + 1) * one_all].cpu().numpy().view(np.int16).reshape(want.shape)
        assert np.array_equal(got, want), "K11 differs from the host route in frame %d of stream %d" % (k % F, k // F)

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

    def row(name, fn, bytes_per_mb):
        ms = timed(fn)
        gbs = bytes_per_mb * mbs * n / (ms * 1e-3) / 1e9
        rows.append({"batch": label, "what": name, "ms": round(ms, 3), "GB/s": round(gbs, 1), "share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 3), "algorithmic_bytes_per_macroblock": bytes_per_mb})

    row("k_pack (K6) I420", lambda: dec.pack_batch(i420.data_ptr(), i420.numel()), 768)
    row("k_side all twelve planes", lambda: dec.side_batch(side.data_ptr(), n * one_all, H.SIDE_ALL), 128 + 12 * 32 + (64 if has_b else 0))
    row("k_side four list-0 motion planes", lambda: dec.side_batch(side.data_ptr(), n * one_l0, L0), 128 + 4 * 32)
    dec.close()
    for r in rows:
        print(json.dumps(r))
    k6 = rows[0]["ms"]
    out = {"batch": label, "frames": n, "size": "%dx%d" % (w, h), "reps": args.reps, "all_planes_over_k_pack": round(rows[1]["ms"] / k6, 3),
           "l0_planes_over_k_pack": round(rows[2]["ms"] / k6, 3), "host_route_ms_scaled_from_%d_frames" % len(picks): round(host_ms, 1),
           "host_route_over_k_side_all": round(host_ms / rows[1]["ms"], 1)}
    out["within_bars"] = out["all_planes_over_k_pack"] <= 1.0 and out["l0_planes_over_k_pack"] <= 0.6
    print(json.dumps(out))
    del i420, side
    torch.cuda.empty_cache()
    return out["within_bars"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--only", default="", help="'ippp' or 'ibbp': one of the two batches")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    ok = True
    if args.only in ("", "ippp"):
        ok &= measure("I P P P", {}, args)
    if args.only in ("", "ibbp"):
        ok &= measure("I B B P", {"bframes": 2, "num_ref_frames": 3}, args)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
