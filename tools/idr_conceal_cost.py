#!/usr/bin/env python3
"""What H264MI_CONCEAL_IDR costs on clean streams when one batch holds several GOPs of a stream: with the bit set an IDR picture that still has a
reference frame is reconstructed in the wave behind that frame instead of in wave 0 (the device learns about damage only after the entropy launch),
so the GOPs of a stream in one batch no longer overlap.  32 streams x 8 GOPs of the bench's 1080p Main CABAC IPPP GOP-30 streams in ONE batch,
decoded with conceal_errors 1 and 17 on the same build in the same process; steady-state frames/s (the marginal rate of bench.timed_fps) of each.
One JSON line.  Usage: idr_conceal_cost.py [--streams 32] [--gops 8] [--steps 3] [--values 1,17,1,17]"""
import argparse
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--gops", type=int, default=8)
    ap.add_argument("--distinct", type=int, default=8, help="distinct GOP streams generated; every stream is a rotation of them")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--values", default="1,17", help="conceal_errors values, measured in this order (a value may repeat)")
    args = ap.parse_args()
    import torch
    import bench
    import h264decode_amd as H
    S, G, F, nd = args.streams, args.gops, args.frames, args.distinct
    with ThreadPoolExecutor(max_workers=bench.generation_threads(nd, 1)) as ex:
        gen = [g[0] for g in ex.map(bench.gen_stream, [(1000 + i, F, args.width, args.height) for i in range(nd)])]
    streams = [b"".join(gen[(s + g) % nd] for g in range(G)) for s in range(S)]
    W, Hc = (args.width + 15) // 16 * 16, (args.height + 15) // 16 * 16
    out = {"workload": "%dx%d Main CABAC IPPP GOP-%d, %d streams x %d GOPs in one batch (%d distinct GOPs), clean, %d steps" % (args.width, args.height, F, S, G, nd, args.steps),
           "runs": []}
    for v in [int(x) for x in args.values.split(",")]:
        dec = H.Decoder(max_streams=S, max_width=W, max_height=Hc, max_frames_per_batch=F * G, max_slices_per_frame=1, max_bitstream_bytes=int(sum(len(s) for s in streams) * 1.1) + (1 << 20),
                        hip_stream=torch.cuda.current_stream().cuda_stream, conceal_errors=v)
        r = bench.timed_fps(dec, streams, S * G * F, args.steps)
        assert all(dec.stream_status(i) == 0 for i in range(S)) and dec.concealed() == (0, 0)
        out["runs"].append({"conceal_errors": v, "steady_fps": r["steady_fps"], "fps": r["fps"], "ms_per_step": r["ms_per_step"]})
        dec.close()
        del dec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
