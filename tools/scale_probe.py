"""K8 (k_scale) next to K6 (k_pack), K7 (k_convert) and the route a caller had before K8: convert to planar RGB at full size, then resize with torch.

    python tools/scale_probe.py [--streams 256] [--distinct 32] [--frames 30] [--reps 5] [--sizes 640x360,224x224]

One process, the bench's clean 1080p batch (bench.gen_stream: the same generator recipe and seeds).  Every figure is the median of --reps launches,
wall clock around launch + synchronise of the decoder's stream (which is torch's current stream here, so the torch route is timed the same way), as
ms and as GB/s of the ALGORITHMIC bytes: the source planes read once (1.5 bytes per source pixel) plus the output written (1.5 or 3 bytes per output
pixel); K6 and K7 as in tools/convert_probe.py.  The route before K8 is convert_batch to "rgbp" at full size followed by
torch.nn.functional.interpolate on the device (bilinear; antialias=True next to the area filter), in float32 chunks, rounded back to uint8: it
computes another rule, so it is compared for time only.  Before timing, K8 at the source's own size is compared with K6 (I420) and K7 (planar RGB)
on the frames of stream 0: the identity of both filters.  If the RGB copy of the batch does not fit beside the decoder, run with fewer --streams."""
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


def torch_resize(rgb, out, ow, oh, antialias, chunk=32):
    """uint8[n, 3, h, w] -> uint8[n, 3, oh, ow] by torch's bilinear interpolation in float32."""
    for a in range(0, rgb.shape[0], chunk):
        v = torch.nn.functional.interpolate(rgb[a:a + chunk].float(), size=(oh, ow), mode="bilinear", align_corners=False, antialias=antialias)
        out[a:a + chunk] = v.round_().clamp_(0, 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="640x360,224x224")
    ap.add_argument("--only", default="", help="under a profiler: launch only the rows whose name contains this (e.g. '640x360 bilinear rgbp'), without the equality checks and the torch route")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    S, F, w, h = args.streams, args.frames, args.width, args.height
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    nd = max(1, min(args.distinct, S))
    with ThreadPoolExecutor(max_workers=min(16, nd)) as ex:
        gen = list(ex.map(bench.gen_stream, [(1000 + i, F, w, h) for i in range(nd)]))
    streams = [gen[i % nd][0] for i in range(S)]
    W, Hc = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    dec = H.Decoder(max_streams=S, max_width=W, max_height=Hc, max_frames_per_batch=F, max_slices_per_frame=1,
                    max_bitstream_bytes=int(sum(len(s) for s in streams) * 1.1) + (1 << 20), hip_stream=torch.cuda.current_stream().cuda_stream)
    dec.decode(streams)
    n, px = S * F, w * h
    omax = max(ow * oh for ow, oh in sizes)
    small = torch.empty((n * 3 * omax,), dtype=torch.uint8, device="cuda")  # every K8 output and the torch route's

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

    def row(name, fn, nbytes, **extra):
        if args.only in name:
            ms = timed(fn)
            rows.append(dict({"what": name, "ms": round(ms, 3), "GB/s": round(nbytes / (ms * 1e-3) / 1e9, 1), "algorithmic_GB": round(nbytes / 1e9, 2)}, **extra))
            return ms
        return None

    def k8_rows():
        out = {}
        for ow, oh in sizes:
            for filt in ("bilinear", "area"):
                for fmt, csc, label in (("i420", 0, "i420"), ("nv12", 0, "nv12"), ("rgb24", 0, "rgb24"), ("rgbp", 0, "rgbp"), ("rgbp", H.CSC_CHROMA_BILINEAR, "rgbp chroma-bilinear")):
                    nbytes = n * (px * 3 // 2 + dec.output_size(fmt, ow, oh))
                    out[(ow, oh, filt, label)] = row("k_scale %dx%d %s %s" % (ow, oh, filt, label), lambda: dec.scale_batch(small.data_ptr(), small.numel(), fmt, (ow, oh), csc, filt), nbytes)
        return out

    if args.only:
        k8_rows()
        dec.close()
        for r in rows:
            print(json.dumps(r))
        return 0

    # the identity first: K8 at the source's own size writes K6's I420 and K7's planar RGB, both filters (stream 0)
    a = torch.empty((F, px * 3 // 2), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    c = torch.empty((F, 3 * px), dtype=torch.uint8, device="cuda")
    d = torch.empty_like(c)
    dec.pack_batch(a.data_ptr(), a.numel(), stream=0)
    dec.convert_batch(c.data_ptr(), c.numel(), "rgbp", 0, stream=0)
    for filt in ("bilinear", "area"):
        dec.scale_batch(b.data_ptr(), b.numel(), "i420", (w, h), 0, filt, stream=0)
        dec.scale_batch(d.data_ptr(), d.numel(), "rgbp", (w, h), 0, filt, stream=0)
        dec.sync()
        assert torch.equal(a, b) and torch.equal(c, d), "k_scale at equal size is not the identity (%s)" % filt
    del a, b, c, d

    i420 = torch.empty((n, px * 3 // 2), dtype=torch.uint8, device="cuda")
    k6 = row("k_pack (K6) I420", lambda: dec.pack_batch(i420.data_ptr(), i420.numel()), n * px * 3)
    del i420
    rgb = torch.empty((n, 3, h, w), dtype=torch.uint8, device="cuda")
    row("k_convert (K7) rgbp nearest", lambda: dec.convert_batch(rgb.data_ptr(), rgb.numel(), "rgbp", 0), n * px * 9 // 2)
    k8 = k8_rows()
    k6_rate = n * px * 3 / (k6 * 1e-3) / 1e9
    route = {}
    for ow, oh in sizes:
        for filt, aa in (("bilinear", False), ("area", True)):
            out = small[:n * 3 * ow * oh].view(n, 3, oh, ow)

            def torch_route():
                dec.convert_batch(rgb.data_ptr(), rgb.numel(), "rgbp", 0)
                torch_resize(rgb, out, ow, oh, aa)
            route[(ow, oh, filt)] = row("convert_batch rgbp + torch interpolate bilinear%s -> %dx%d (the route before K8, next to %s)" % (", antialias" if aa else "", ow, oh, filt),
                                        torch_route, n * (px * 3 // 2 + 3 * ow * oh))
    dec.close()
    for r in rows:
        print(json.dumps(r))
    ahead = all(ms < route[key[:3]] for key, ms in k8.items())
    print(json.dumps({"frames": n, "size": "%dx%d" % (w, h), "reps": args.reps, "k_pack_GB/s": round(k6_rate, 1), "every_k_scale_configuration_beats_the_torch_route": ahead,
                      "below_half_of_k_pack_rate": [r["what"] for r in rows if r["what"].startswith("k_scale") and r["GB/s"] < k6_rate / 2]}))
    return 0 if ahead else 1


if __name__ == "__main__":
    sys.exit(main())
