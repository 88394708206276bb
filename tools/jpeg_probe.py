"""K13 (k_jpeg) next to K6 (k_pack) over the same frames, and next to Pillow's encoder on a host core.

    python tools/jpeg_probe.py [--streams 16] [--distinct 8] [--frames 16] [--reps 11]

One process, the bench's clean 1080p batch (bench.gen_stream: the same generator recipe and seeds), as tools/stats_probe.py.  Every figure is the median
of --reps calls, wall clock around the call (three launches: sizing, scan, writing) + synchronise of the decoder's stream, as ms and as GB/s of SOURCE
bytes read once (1.5 a pixel; the kernel reads them twice).  1, 32 and 256 items (streams x frames must reach 256), at quality 75 and 90, with restart_mcus
0 (an MCU row per interval: 68 wavefronts a frame) and 8 (8 MCUs: 1020 wavefronts a frame).  A slot is the header plus w * h bytes, which no item of
this material exceeds (checked: every status is 0).  Before timing, the first file of every configuration is opened with Pillow and its luma held to
K6's frame (PSNR above 30 dB).  For context: Pillow's own encode of one such frame (quality alike, 4:2:0) on a host core, the planes already in host
memory -- the route this replaces also copies 3 MB a frame over PCIe first."""
import argparse
import ctypes
import io
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
from h264decode_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU: there is nothing to report without one"
    from PIL import Image
    S, F, w, h = args.streams, args.frames, args.width, args.height
    nd = max(1, min(args.distinct, S))
    with ThreadPoolExecutor(max_workers=min(16, nd)) as ex:
        gen = list(ex.map(bench.gen_stream, [(1000 + i, F, w, h) for i in range(nd)]))
    streams = [gen[i % nd][0] for i in range(S)]
    W, Hc = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    dec = H.Decoder(max_streams=S, max_width=W, max_height=Hc, max_frames_per_batch=F, max_slices_per_frame=1,
                    max_bitstream_bytes=int(sum(len(s) for s in streams) * 1.1) + (1 << 20), hip_stream=torch.cuda.current_stream().cuda_stream)
    dec.decode(streams)
    n_all, px = S * F, w * h
    counts = [c for c in (1, 32, 256) if c <= n_all]
    slot = (H.jpeg_size(w, h)[0] + px + 15) & ~15
    out = torch.empty(((16 * n_all + 255) & ~255) + n_all * slot, dtype=torch.uint8, device="cuda")
    i420 = torch.empty((n_all, px * 3 // 2), dtype=torch.uint8, device="cuda")
    arr = (_lib.JpegItem * n_all)()
    for i, a in enumerate(arr):
        a.stream, a.frame = i // F, i % F

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

    def row(what, ms, n, **more):
        r = dict(what=what, items=n, ms=round(ms, 3), ms_per_item=round(ms / n, 4))
        r["GB/s_source"] = round(1.5 * px * n / (ms * 1e-3) / 1e9, 1)
        r.update(more)
        print(json.dumps(r), flush=True)

    dec.pack_batch(i420.data_ptr(), i420.numel())
    dec.sync()
    first = i420[0].cpu().numpy()
    for n in counts:
        def k6():
            for i in range(n):  # K6 over the same frames: the frame call, item by item (the batch call takes whole streams)
                _lib.check(dec._L.h264mi_frame_pack_device(dec._h, arr[i].stream, arr[i].frame, i420.data_ptr() + i * i420.shape[1], i420.shape[1]))
        if n == n_all:
            row("k_pack (K6) I420, one launch", timed(lambda: dec.pack_batch(i420.data_ptr(), i420.numel())), n)
        else:
            row("k_pack (K6) I420, a launch per frame", timed(k6), n)
        for quality in (75, 90):
            for restart in (0, 8):
                spec = H.jpeg_spec(quality, "keep", restart)

                def k13():
                    got = ctypes.c_size_t(0)
                    _lib.check(dec._L.h264mi_items_jpeg_device(dec._h, ctypes.byref(spec), arr, n, slot, out.data_ptr(), out.numel(), ctypes.byref(got)))
                ms = timed(k13)
                head = (16 * n + 255) & ~255
                res = out[:16 * n].cpu().numpy().view(np.uint32).reshape(n, 4)
                assert (res[:, 1] == 0).all(), "an item did not fit its slot"
                im = Image.open(io.BytesIO(out[head:head + int(res[0, 0])].cpu().numpy().tobytes()))
                im.draft("YCbCr", im.size)
                luma = np.asarray(im)[:, :, 0].astype(np.float64)
                psnr = 10 * np.log10(255.0 ** 2 / max(np.mean((luma - first[:px].reshape(h, w)) ** 2), 1e-9))
                assert im.size == (w, h) and psnr > 30, psnr
                row("k_jpeg (K13) quality %d restart_mcus %d" % (quality, restart), ms, n, mean_file_bytes=int(res[:, 0].mean()), luma_psnr_db_first=round(psnr, 2))
    # the host route's encoder alone, one frame, one core
    cw, ch = (w + 1) // 2, (h + 1) // 2
    planes = [first[:px].reshape(h, w), first[px:px + cw * ch].reshape(ch, cw), first[px + cw * ch:].reshape(ch, cw)]
    up = [np.repeat(np.repeat(c, 2, 0), 2, 1)[:h, :w] for c in planes[1:]]
    img = Image.merge("YCbCr", [Image.fromarray(np.ascontiguousarray(p)) for p in [planes[0]] + up])
    for quality in (75, 90):
        ms = []
        for _ in range(args.reps):
            f = io.BytesIO()
            t0 = time.perf_counter()
            img.save(f, "JPEG", quality=quality, subsampling=2)
            ms.append((time.perf_counter() - t0) * 1e3)
        row("Pillow (libjpeg) on a host core, quality %d" % quality, statistics.median(ms), 1, file_bytes=len(f.getvalue()))
    dec.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
