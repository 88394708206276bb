"""K7 (k_convert) next to K6 (k_pack) and next to the route a caller had before K7: pack to I420, then colour-convert with torch element-wise ops.

    python tools/convert_probe.py [--streams 256] [--distinct 32] [--frames 30] [--reps 5]

One process, the bench's clean 1080p batch (bench.gen_stream: the same generator recipe and seeds).  Every figure is the median of --reps launches,
wall clock around launch + synchronise of the decoder's stream (which is torch's current stream here, so the torch route is timed the same way), as
ms and as GB/s of the ALGORITHMIC bytes: 2 x 1.5 bytes per pixel for K6 and NV12, 1.5 + 3 for RGB; the torch route is charged the same 1.5 + 3 although
it moves several times that.  Before timing, K7's planar RGB is compared with the torch route's (the same integer rule) and its NV12 with K6's I420.
If the RGB copy of the batch does not fit beside the decoder, run with fewer --streams."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import h264decode_amd as H  # noqa: E402

COEFFS = {(1, 0): (9539, 13075, 3209, 6660, 16525), (1, 1): (8192, 11485, 2819, 5850, 14516),
          (2, 0): (9539, 14686, 1747, 4366, 17305), (2, 1): (8192, 12901, 1535, 3835, 15201)}  # H264MI_CSC_COEFFS


def torch_rgbp(packed, out, n, w, h, matrix, full, chunk=16):
    """The rule of include/h264mi.h (nearest chroma) in torch element-wise ops over tight I420 frames: packed uint8[n, w*h*3/2] -> out uint8[n, 3, h, w]."""
    cy, crv, cgu, cgv, cbu = COEFFS[(matrix, full)]
    wc, hc = w // 2, h // 2
    for a in range(0, n, chunk):
        p = packed[a:a + chunk]
        m = p.shape[0]
        y = p[:, :w * h].view(m, h, w).to(torch.int32)
        cb = p[:, w * h:w * h + wc * hc].view(m, hc, wc).to(torch.int32) - 128
        cr = p[:, w * h + wc * hc:].view(m, hc, wc).to(torch.int32) - 128
        u = cb.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        v = cr.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        t = cy * (y - (0 if full else 16)) + 4096
        o = out[a:a + chunk]
        o[:, 0] = ((t + crv * v) >> 13).clamp_(0, 255).to(torch.uint8)
        o[:, 1] = ((t - cgu * u - cgv * v) >> 13).clamp_(0, 255).to(torch.uint8)
        o[:, 2] = ((t + cbu * u) >> 13).clamp_(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="under a profiler: launch only the rows whose name contains this (e.g. 'rgb24 nearest'), without the equality checks and the torch route")
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
    rgb = torch.empty((n, 3, h, w), dtype=torch.uint8, device="cuda")
    ref = torch.empty((min(n, 32), 3, h, w), dtype=torch.uint8, device="cuda")

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
            rows.append({"what": name, "ms": round(ms, 3), "GB/s": round(bytes_per_px * px * n / (ms * 1e-3) / 1e9, 1), "algorithmic_bytes_per_pixel": bytes_per_px})

    def kernel_rows():
        row("k_pack (K6) I420", lambda: dec.pack_batch(i420.data_ptr(), i420.numel()), 3.0)
        row("k_convert NV12", lambda: dec.convert_batch(i420.data_ptr(), i420.numel(), "nv12", 0), 3.0)
        for fmt in ("rgb24", "rgbp"):
            for name, csc in (("nearest", 0), ("bilinear", H.CSC_CHROMA_BILINEAR)):
                row("k_convert %s %s" % (fmt, name), lambda: dec.convert_batch(rgb.data_ptr(), rgb.numel(), fmt, csc), 4.5)
    if args.only:
        kernel_rows()
        dec.close()
        for r in rows:
            print(json.dumps(r))
        return 0

    # the same bytes first: K7 planar RGB == the torch route on K6's frames (BT.709 limited, what AUTO resolves 1080p to), K7 NV12 luma == K6 luma
    dec.pack_batch(i420.data_ptr(), i420.numel())
    dec.convert_batch(rgb.data_ptr(), rgb.numel(), "rgbp", 0)
    dec.sync()
    torch_rgbp(i420, ref, ref.shape[0], w, h, 2, 0)
    torch.cuda.synchronize()
    assert torch.equal(ref, rgb[:ref.shape[0]]), "k_convert and the torch route disagree"
    nv = torch.empty_like(i420)
    dec.convert_batch(nv.data_ptr(), nv.numel(), "nv12", 0)
    dec.sync()
    assert torch.equal(nv[:, :px], i420[:, :px]) and torch.equal(nv[:, px::2], i420[:, px:px + px // 4]) and torch.equal(nv[:, px + 1::2], i420[:, px + px // 4:])
    del nv, ref

    kernel_rows()

    def torch_route():
        dec.pack_batch(i420.data_ptr(), i420.numel())
        torch_rgbp(i420, rgb, n, w, h, 2, 0)
    row("pack_batch + torch element-wise ops -> rgbp nearest (the route before K7)", torch_route, 4.5)
    dec.close()
    for r in rows:
        print(json.dumps(r))
    slowest = max(r["ms"] for r in rows if r["what"].startswith("k_convert"))
    print(json.dumps({"frames": n, "size": "%dx%d" % (w, h), "reps": args.reps, "every_k_convert_format_beats_the_torch_route": slowest < rows[-1]["ms"]}))
    return 0 if slowest < rows[-1]["ms"] else 1


if __name__ == "__main__":
    sys.exit(main())
