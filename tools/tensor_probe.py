"""K9 (k_tensor) next to K6 (k_pack), K8 (k_scale) and the route a caller had before K9: frames_tensor(size=...) to uint8 RGB, then torch.

    python tools/tensor_probe.py [--streams 256] [--distinct 32] [--frames 30] [--reps 5] [--only a,b,...]

One process, the bench's clean 1080p batch (bench.gen_stream: the same generator recipe and seeds).  Every figure is the median of --reps runs, wall
clock around call + synchronise of the decoder's stream (torch's current stream here, so the torch route is timed the same way).  Per configuration
three rows: the K9 launch alone into a buffer that exists (ms, and GB/s of the ALGORITHMIC bytes: the region's source planes read once, 1.5 bytes per
source pixel, plus the item written), frames_tensor with the model keywords (K9 + the allocation and the two synchronisations), and the route before
K9 -- frames_tensor(size=(sw, sh)) to uint8, then .to(dtype), a multiply, an add, a permute for HWC and F.pad for the letterbox bands; for the regions
(d), which K8 cannot cut, convert_batch to planar RGB at full size followed by torch.nn.functional.interpolate of the four slices (bilinear: it
computes another rule, so it is compared for time only).  The configurations:
  a  640x640 letterbox f16 CHW           b  224x224 stretch f32 CHW, ImageNet mean / std, bilinear and area          c  224x224 stretch bf16 HWC
  d  four 256x256 regions per frame -> 112x112 f16 CHW          e  640x360 stretch u8 CHW: K8's bytes, next to k_scale rgbp
Before timing, (e) is compared with K8's output on stream 0: the same bytes."""
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

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ELEM = {torch.uint8: 1, torch.float16: 2, torch.bfloat16: 2, torch.float32: 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated configuration letters; under a profiler also skips the routes (--no-routes)")
    ap.add_argument("--no-routes", action="store_true")
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
    dev = "cuda:%d" % dec.device

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

    def row(name, fn, nbytes=None):
        ms = timed(fn)
        r = {"what": name, "ms": round(ms, 3)}
        if nbytes:
            r.update({"GB/s": round(nbytes / (ms * 1e-3) / 1e9, 1), "algorithmic_GB": round(nbytes / 1e9, 2)})
        rows.append(r)
        print(json.dumps(r), flush=True)
        return ms

    scale = torch.tensor([1.0 / (255.0 * s) for s in STD], dtype=torch.float32, device=dev)
    bias = torch.tensor([-m / s for m, s in zip(MEAN, STD)], dtype=torch.float32, device=dev)

    def route(size, dtype, fmt="rgbp", filter="bilinear", canvas=None, norm=True):
        """What a caller does without K9: K8 to uint8 at the picture size, then torch -- every step another pass over the batch."""
        t = dec.frames_tensor(-1, fmt, 0, size=size, filter=filter)
        shp = (1, 3, 1, 1) if fmt == "rgbp" else (1, 1, 1, 3)
        t = t.to(dtype)
        if norm:
            t = t * scale.to(dtype).view(shp) + bias.to(dtype).view(shp)
        else:
            t = t * (1.0 / 255.0)
        if canvas is not None:
            py = (canvas[1] - size[1]) // 2
            px_ = (canvas[0] - size[0]) // 2
            t = torch.nn.functional.pad(t, (px_, canvas[0] - size[0] - px_, py, canvas[1] - size[1] - py), value=114.0 / 255.0)
        return t

    only = set(args.only.split(",")) if args.only else set("abcde")
    verdict = {}

    def config(letter, label, kw, src_px, route_fn, out_shape, dtype):
        """kw: the model keywords of frames_tensor; src_px: source pixels read per item."""
        if letter not in only:
            return
        items = out_shape[0]
        nbytes = items * (src_px * 3 // 2) + int(torch.Size(out_shape).numel()) * ELEM[dtype]
        out = torch.empty(out_shape, dtype=dtype, device=dev)
        fmt = kw.get("fmt", "rgbp")
        sc = [1.0 / (255.0 * s) for s in STD] if kw.get("norm", True) else [1.0 / 255.0] * 3
        bi = [-m / s for m, s in zip(MEAN, STD)] if kw.get("norm", True) else [0.0] * 3
        if dtype == torch.uint8:
            sc, bi = [1.0] * 3, [0.0] * 3
        spec = H.tensor_spec(kw["size"], fmt, dtype, 0, kw.get("filter", "bilinear"), kw.get("letterbox", False), False, (114, 114, 114), sc, bi)
        cap = out.numel() * out.element_size()
        rois = kw.get("rois")
        if rois:  # the item table built once: the row is the launch, not Python filling 30 000 structs (frames_tensor's row below includes that)
            arr = (H._lib.TensorItem * len(rois))(*[H._lib.TensorItem(*r) for r in rois])
            got = ctypes.c_size_t(0)

            def launch():
                H._lib.check(dec._L.h264mi_items_tensor_device(dec._h, ctypes.byref(spec), arr, len(rois), out.data_ptr(), cap, ctypes.byref(got)))
        else:
            def launch():
                dec.tensor_batch(out.data_ptr(), cap, spec)
        k9 = row("k_tensor %s: %s (the launch)" % (letter, label), launch, nbytes)
        del out
        extra = dict(scale=sc, bias=bi) if dtype != torch.uint8 else {}
        ft = row("frames_tensor %s: %s (K9, allocation and synchronisations included)" % (letter, label),
                 lambda: dec.frames_tensor(-1, fmt, 0, size=kw["size"], filter=kw.get("filter", "bilinear"), dtype=dtype, letterbox=kw.get("letterbox", False), rois=rois, **extra))
        if not args.no_routes:
            rt = row("route before K9 %s: %s" % (letter, label), route_fn)
            verdict["%s %s" % (letter, label)] = {"k_tensor_ms": round(k9, 3), "frames_tensor_ms": round(ft, 3), "route_ms": round(rt, 3), "ahead": ft < rt}
        torch.cuda.empty_cache()

    # references in the same run
    i420 = torch.empty((n, px * 3 // 2), dtype=torch.uint8, device=dev)
    k6 = row("k_pack (K6) I420", lambda: dec.pack_batch(i420.data_ptr(), i420.numel()), n * px * 3)
    del i420
    k6_rate = n * px * 3 / (k6 * 1e-3) / 1e9
    small = torch.empty((n, 3, 360, 640), dtype=torch.uint8, device=dev)
    row("k_scale (K8) 640x360 bilinear rgbp", lambda: dec.scale_batch(small.data_ptr(), small.numel(), "rgbp", (640, 360), 0, "bilinear"), n * (px * 3 // 2 + 3 * 640 * 360))
    if "e" in only:  # K9's u8 planes at 640x360 are K8's bytes
        dec.sync()
        assert torch.equal(dec.frames_tensor(0, "rgbp", 0, size=(640, 360), dtype=torch.uint8, letterbox=False, bgr=False, rois=[(0, f, 0, 0, 0, 0) for f in range(F)]), small[:F]), "K9 u8 is not K8"
    del small
    torch.cuda.empty_cache()

    config("a", "640x640 letterbox f16 CHW", dict(size=(640, 640), letterbox=True, norm=False), px,
           lambda: route((640, 360), torch.float16, canvas=(640, 640), norm=False), (n, 3, 640, 640), torch.float16)
    config("b", "224x224 stretch f32 CHW ImageNet bilinear", dict(size=(224, 224)), px, lambda: route((224, 224), torch.float32), (n, 3, 224, 224), torch.float32)
    config("b", "224x224 stretch f32 CHW ImageNet area", dict(size=(224, 224), filter="area"), px, lambda: route((224, 224), torch.float32, filter="area"), (n, 3, 224, 224),
           torch.float32)
    config("c", "224x224 stretch bf16 HWC ImageNet", dict(size=(224, 224), fmt="rgb24"), px, lambda: route((224, 224), torch.bfloat16, fmt="rgb24"), (n, 224, 224, 3),
           torch.bfloat16)
    if "d" in only:
        boxes = [(320, 160), (960, 160), (320, 600), (960, 600)]  # four 256x256 regions of every frame
        rois = [(s, f, x, y, 256, 256) for s in range(S) for f in range(F) for x, y in boxes]
        rgb = None if args.no_routes else torch.empty((n, 3, h, w), dtype=torch.uint8, device=dev)

        def regions_route():
            # K8 cannot cut regions and 4 n scale_frame calls on cropped copies would be 4 n launches: the cheapest route is K7 at full size, then torch
            # per box over the whole batch (slice, float, interpolate, normalise)
            dec.convert_batch(rgb.data_ptr(), rgb.numel(), "rgbp", 0)
            out = torch.empty((n, 4, 3, 112, 112), dtype=torch.float16, device=dev)
            for b_, (x, y) in enumerate(boxes):
                for a in range(0, n, 512):
                    v = torch.nn.functional.interpolate(rgb[a:a + 512, :, y:y + 256, x:x + 256].float(), size=(112, 112), mode="bilinear", align_corners=False)
                    out[a:a + 512, b_] = (v.round_().clamp_(0, 255) * scale.view(1, 3, 1, 1) + bias.view(1, 3, 1, 1)).to(torch.float16)
            return out
        config("d", "four 256x256 regions per frame -> 112x112 f16 CHW ImageNet", dict(size=(112, 112), rois=rois), 256 * 256, regions_route, (4 * n, 3, 112, 112), torch.float16)
        del rgb
    config("e", "640x360 stretch u8 CHW (K8's bytes)", dict(size=(640, 360)), px, lambda: dec.frames_tensor(-1, "rgbp", 0, size=(640, 360)), (n, 3, 360, 640), torch.uint8)
    dec.close()
    ahead = all(v["ahead"] for v in verdict.values())
    print(json.dumps({"frames": n, "size": "%dx%d" % (w, h), "reps": args.reps, "k_pack_GB/s": round(k6_rate, 1), "configurations": verdict,
                      "every_configuration_beats_the_route_before_K9": ahead,
                      "below_half_of_k_pack_rate": [r["what"] for r in rows if r["what"].startswith("k_tensor") and r.get("GB/s", 1e9) < k6_rate / 2]}))
    return 0 if ahead or args.no_routes else 1


if __name__ == "__main__":
    sys.exit(main())
