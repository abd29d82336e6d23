#!/usr/bin/env python
"""Node-wide SVGF (atn_mgpu_svgf_render, docs/MGPU_SVGF.md) on BASELINE config 5's shape -- sponza_lod, 1080p, 1 spp, 5 bounces, SVGF
frames with compute_motion = 1 -- beside the single context it must equal: tools/skin_bench.py's window protocol.

  single          atn_svgf_render on one PathTracing context                        (the yardstick, same process)
  mgpu N          atn_mgpu_svgf_render on N shards, N in --shards (default 1, 2, 4, 8)

each with every count of --frames-in-flight (default 1 and 4).  The shards go to devices 0 .. N-1 when the box has that many GPUs;
otherwise they all share device 0 (an ordinal may repeat), and then N > 1 measures what the seam COSTS -- N worker threads, N path
passes of 1/N of the frame each on one GPU, the pack, the copies, the unpack -- not a speed-up.  The result says which of the two it was.

ms per frame: a host clock around `--frames` frames that end in a device synchronise, `--repeats` windows per configuration, the
configurations taken in turn inside one process; median, min and max of the windows.  The two kernels of the exchange: HIP-event time
per launch (destination.profile = 1, atn_mgpu_get_kernel_times) over `--profiled` frames of a pass of their own, one frame in flight --
k_svgf_pack_tiles on shard 1, k_svgf_unpack_tiles on shard 0 -- with the bytes they move and the rate that makes.

    python tools/mgpu_svgf_bench.py [--frames 30] [--warmup 4] [--repeats 5] [--profiled 20] [--shards 1,2,4,8] [--frames-in-flight 1,4]
                                    [--out profiles/mgpu_svgf_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1920, 1080
DEPTH, RR = 5, 3
EXCHANGE_BYTES_PER_PIXEL = 4 * 16       # contributions, normal+depth, albedo+id, primary position


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profiled", type=int, default=20)
    ap.add_argument("--shards", default="1,2,4,8")
    ap.add_argument("--frames-in-flight", default="1,4")
    ap.add_argument("--out", default=os.path.join("profiles", "mgpu_svgf_bench.json"))
    args = ap.parse_args()
    shard_counts = [int(x) for x in args.shards.split(",")]
    in_flight = [int(x) for x in args.frames_in_flight.split(",")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mgpu_svgf_bench: no GPU (there is nothing to measure without one)")
    torch.cuda.init()
    visible = torch.cuda.device_count()
    from aten_amd.renderer import MultiGpuPathTracing, PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    fs, cam = scenedefs.sponza_lod()
    camera = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)

    def devices(n):
        return list(range(n)) if visible >= n else [0] * n

    def setup(r):
        r.UpdateSceneData(fs)
        r.updateCamera(camera)
        r.initSampler(W, H, 0)
        return r

    renderers = {"single": setup(PathTracing(0))}
    for n in shard_counts:
        renderers["mgpu_%d" % n] = setup(MultiGpuPathTracing(devices(n)))
    frame = {k: 0 for k in renderers}

    def one(name, profile=False):
        renderers[name].svgf_render(W, H, DEPTH, RR, frame=frame[name], compute_motion=1, download=False, profile=profile)
        frame[name] += 1

    windows = {}
    for fif in in_flight:
        for name, r in renderers.items():
            r.set_frames_in_flight(fif)
            for _ in range(args.warmup):
                one(name)
            r.synchronize()
        for _ in range(args.repeats):
            for name, r in renderers.items():
                one(name)
                r.synchronize()
                t = time.perf_counter()
                for _ in range(args.frames):
                    one(name)
                r.synchronize()
                windows.setdefault((name, fif), []).append((time.perf_counter() - t) / args.frames * 1e3)

    # the two kernels of the exchange, in a pass of their own (event brackets around every launch slow the frame down)
    kernels = {}
    for n in shard_counts:
        if n < 2:
            continue
        name = "mgpu_%d" % n
        m = renderers[name]
        m.set_frames_in_flight(1)
        one(name, profile=True)
        m.reset_kernel_times()
        for _ in range(args.profiled):
            one(name, profile=True)
        pack_ms, pack_n = m.kernel_times(1)["svgf_pack"]
        unpack_ms, unpack_n = m.kernel_times(0)["svgf_unpack"]
        pack_b = EXCHANGE_BYTES_PER_PIXEL * W * H / n * 2           # one shard's pixels, read and written once each
        unpack_b = EXCHANGE_BYTES_PER_PIXEL * W * H * (n - 1) / n * 2
        pk, up = pack_ms / max(pack_n, 1), unpack_ms / max(unpack_n, 1)
        kernels[name] = dict(pack_ms=round(pk, 4), pack_launches=pack_n, pack_megabytes=round(pack_b / 1e6, 1),
                             pack_gigabytes_per_second=round(pack_b / 1e6 / pk, 1) if pk > 0 else None,
                             unpack_ms=round(up, 4), unpack_launches=unpack_n, unpack_megabytes=round(unpack_b / 1e6, 1),
                             unpack_gigabytes_per_second=round(unpack_b / 1e6 / up, 1) if up > 0 else None)
    for r in renderers.values():
        r.close()

    def stats(w):
        return dict(median=round(float(np.median(w)), 4), min=round(min(w), 4), max=round(max(w), 4))
    shared = [n for n in shard_counts if visible < n]
    out = dict(workload="sponza_lod %dx%d 1 spp %d bounces, SVGF frames (compute_motion = 1)" % (W, H, DEPTH),
               protocol="%d warm-up frames, %d timed per window, %d windows per configuration taken in turn in one process; kernels: HIP events over %d profiled frames, one frame in flight"
                        % (args.warmup, args.frames, args.repeats, args.profiled),
               visible_gpus=visible,
               shards_sharing_device_0=shared,
               note=("shard counts %s share ONE GPU here: their figures are the overhead of the seam, not a speed-up" % shared) if shared else "every shard on a GPU of its own",
               exchange_megabytes_per_frame={"mgpu_%d" % n: round(EXCHANGE_BYTES_PER_PIXEL * W * H * (n - 1) / n / 1e6, 1) for n in shard_counts},
               ms_per_frame={"%s, %d in flight" % k: stats(w) for k, w in windows.items()},
               exchange_kernels=kernels)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
