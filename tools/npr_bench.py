#!/usr/bin/env python
"""NPR frame cost (atn_npr_render) on npr_sponza (sponza_lod, GGX materials, feature lines on every material), 1080p, 1 spp,
5 bounces, one frame in flight, beside atn_render on the same scene.  Prints one JSON line.

ms per frame: device events (torch.cuda.Event on the context's own stream) around `--steps` frames after `--warmup`, repeated
`--repeats` times (median and spread).  Mrays/s is the reference's definition, W * H * spp / ms.

    python tools/npr_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--width 1920 --height 1080] [--dump-outputs DIR]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--dump-outputs", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    W, H = args.width, args.height
    fs, cam = scenedefs.npr_sponza()
    c = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)
    r = PathTracing(0)
    r.UpdateSceneData(fs)
    r.updateCamera(c)
    r.initSampler(W, H, 0)
    r._l.atn_stream.restype = C.c_void_p
    stream = torch.cuda.ExternalStream(r._l.atn_stream(r._ctx))
    frame = [0]

    def timed(step):
        for _ in range(args.warmup):
            step()
        out = []
        for _ in range(args.repeats):
            r._l.atn_synchronize(r._ctx)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                step()
            e1.record(stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / args.steps)
        return out

    def npr_step():
        r.npr_render(W, H, max_depth=args.depth, frame=frame[0], download=False)
        frame[0] += 1

    def pt_step():
        r.render(W, H, max_depth=args.depth, frame=frame[0], download=False)
        frame[0] += 1

    res = {"metric": "ms per NPR frame (npr_sponza, %dx%d, 1 spp, %d bounces, 1 frame in flight)" % (W, H, args.depth),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    films = {}
    for name, step in (("npr", npr_step), ("path_tracer", pt_step)):
        r.npr_reset()
        frame[0] = 0
        ms = timed(step)
        res["cases"][name] = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                              "mrays_per_s": round(W * H / 1e6 / (float(np.median(ms)) / 1e3), 3)}
        if args.dump_outputs:
            r.npr_reset()
            films[name] = (r.npr_render if name == "npr" else r.render)(W, H, max_depth=args.depth, frame=0, progressive=False)
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for k, v in films.items():
            np.save(os.path.join(args.dump_outputs, "npr_bench_%s.npy" % k), v[::4, ::4, :3].astype(np.float32))     # every 4th pixel
    r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
