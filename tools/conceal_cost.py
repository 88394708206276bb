#!/usr/bin/env python3
"""What error concealment (h264mi_config.conceal_errors) costs on the bench workload: the 1080p Main CABAC GOP-30 batch of bench.py
(same streams, same scratch cache, same timed region: K passes of execute over a batch resident in HBM) decoded

    off      with the switch off                      (what bench.py measures)
    clean    with the switch on, intact streams       (k_conceal launched, nothing to do)
    damaged  with the switch on, the slice data of about --permille of the P slices zeroed
             (the streams have one slice per picture: a failed slice conceals the whole picture)
    lost     with H264MI_CONCEAL_PICTURES on top, about --permille of the non-IDR reference pictures REMOVED: every one of them is a frame_num gap
             that the decoder fills with an inserted frame (frames/s counts output frames, so the inserted ones are included)

and prints one JSON line with frames/s of each.  For the duration of k_conceal per pass run one mode under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/conceal_cost.py --modes damaged --steps 2
"""
import argparse
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def damage(stream, permille, rnd):
    """The stream with the slice data of about `permille` of its non-IDR slices replaced by zero bytes (tests/concealutil.zeroed_unit)."""
    import concealutil as cu
    units, slices, _ = cu.parse(stream)
    n = 0
    for s in slices:
        if s.type == 1 and rnd.random() * 1000 < permille:
            units[s.unit] = cu.zeroed_unit(s, units[s.unit][:cu._sc_len(units[s.unit])])
            n += 1
    return b"".join(units), n


def lose(stream, permille, rnd):
    """The stream without about `permille` of its non-IDR reference pictures (never the last picture: something has to reveal the gap)."""
    import concealutil as cu
    units, _, pics = cu.parse(stream)
    n = 0
    for p in pics[1:-1]:
        if p[0].type == 1 and p[0].ref_idc and rnd.random() * 1000 < permille:
            for s in p:
                units[s.unit] = b""
            n += 1
    return b"".join(units), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--permille", type=float, default=10.0, help="share of the P slices that are damaged")
    ap.add_argument("--modes", default="off,clean,damaged,lost")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import torch
    import bench
    import h264decode_amd as H
    S, F, nd = args.streams, args.frames, min(args.distinct, args.streams)
    with ThreadPoolExecutor(max_workers=bench.generation_threads(nd, 1)) as ex:
        gen = list(ex.map(bench.gen_stream, [(1000 + i, F, args.width, args.height) for i in range(nd)]))
    W, Hc = (args.width + 15) // 16 * 16, (args.height + 15) // 16 * 16
    rnd = random.Random(args.seed)
    out = {"workload": "%dx%d Main CABAC IPPP GOP-%d, %d streams (%d distinct), %d steps" % (args.width, args.height, F, S, nd, args.steps), "modes": {}}
    for mode in args.modes.split(","):
        n_damaged = 0
        streams = [gen[i % nd][0] for i in range(S)]
        if mode == "damaged":
            dm = [damage(g[0], args.permille, rnd) for g in gen]
            streams = [dm[i % nd][0] for i in range(S)]
            n_damaged = sum(dm[i % nd][1] for i in range(S))
        if mode == "lost":
            dm = [lose(g[0], args.permille, rnd) for g in gen]
            streams = [dm[i % nd][0] for i in range(S)]
            n_damaged = sum(dm[i % nd][1] for i in range(S))
        dec = H.Decoder(max_streams=S, max_width=W, max_height=Hc, max_frames_per_batch=F, max_slices_per_frame=1, max_bitstream_bytes=int(sum(len(s) for s in streams) * 1.1) + (1 << 20),
                        hip_stream=torch.cuda.current_stream().cuda_stream, conceal_errors=0 if mode == "off" else (H.CONCEAL_SLICES | H.CONCEAL_PICTURES if mode == "lost" else H.CONCEAL_SLICES))
        info = dec.prepare(streams)
        assert info.n_frames == S * F
        for _ in range(args.warmup):
            dec.execute()
        dec.sync()
        torch.cuda.synchronize()
        before, pics_before = dec.concealed(), dec.concealed_pictures()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            dec.execute()
        dec.sync()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        after = dec.concealed()
        out["modes"][mode] = {"frames_per_s": round(S * F * args.steps / dt, 1), "ms_per_step": round(dt / args.steps * 1e3, 3), ("lost_pictures_in_batch" if mode == "lost" else "damaged_slices_in_batch"): n_damaged,
                              "inserted_pictures_last_pass": dec.concealed_pictures() - pics_before,
                              "concealed_slices_last_pass": after[0] - before[0], "concealed_macroblocks_last_pass": after[1] - before[1],
                              "stream_status_errors": sum(1 for i in range(S) if dec.stream_status(i) != 0)}
        dec.close()
        del dec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
