#!/usr/bin/env python
"""What the NPR look-through (atn_npr_set_skip_through, docs/NPR_ADVANCE.md) costs per NPR frame on npr_sponza, 1080p, 1 spp,
5 bounces, one frame in flight.  tools/npr_bench.py's protocol; three cases, a fresh context each:

  mode0          skip-through off: the frame as it was
  mode1_no_work  skip-through on, the scene unchanged: nothing to look through, nothing new is launched
  mode1_alpha    skip-through on, alpha blending on and the scene's largest material (most triangles) at baseColor.a = 0.5

ms per frame: device events (torch.cuda.Event on the context's own stream) around `--steps` frames after `--warmup`, repeated
`--repeats` times (median and spread).  Prints one JSON line.  The per-kernel split is a run of its own:
rocprofv3 --kernel-trace --stats -- python tools/npr_advance_bench.py --only mode1_alpha.

    python tools/npr_advance_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--width 1920 --height 1080] [--only CASE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = ("mode0", "mode1_no_work", "mode1_alpha")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--only", choices=CASES, default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    W, H = args.width, args.height
    res = {"metric": "ms per NPR frame (npr_sponza, %dx%d, 1 spp, %d bounces, 1 frame in flight)" % (W, H, args.depth),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    for name in CASES:
        if args.only and name != args.only:
            continue
        fs, cam = scenedefs.npr_sponza()
        extra = {}
        if name == "mode1_alpha":
            tri_mtrl = fs.arrays["triangles"]["mtrlid"]
            big = int(np.bincount(tri_mtrl[tri_mtrl >= 0]).argmax())
            fs.arrays["materials"]["baseColor"][big][3] = 0.5
            fs.desc.config.enable_alpha_blending = 1
            extra = {"material": big, "triangles_of_it": int((tri_mtrl == big).sum()), "triangles": int(len(tri_mtrl))}
        c = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)
        r = PathTracing(0)
        r.UpdateSceneData(fs)
        r.updateCamera(c)
        r.initSampler(W, H, 0)
        r.npr_set_skip_through(0 if name == "mode0" else 1)
        r._l.atn_stream.restype = C.c_void_p
        stream = torch.cuda.ExternalStream(r._l.atn_stream(r._ctx))
        frame = 0
        for _ in range(args.warmup):
            r.npr_render(W, H, max_depth=args.depth, frame=frame, download=False)
            frame += 1
        ms = []
        for _ in range(args.repeats):
            r._l.atn_synchronize(r._ctx)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                r.npr_render(W, H, max_depth=args.depth, frame=frame, download=False)
                frame += 1
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        res["cases"][name] = dict({"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                                   "mrays_per_s": round(W * H / 1e6 / (float(np.median(ms)) / 1e3), 3)}, **extra)
        if name == "mode1_alpha":
            # how many primary paths looked through something in the last frame (the stage buffer, one more frame)
            r.npr_capture(True)
            r.npr_render(W, H, max_depth=args.depth, frame=frame, download=False)
            res["cases"][name]["primary_paths_looking_through"] = float((r.npr_advance_buffer()["kind"] > 0).mean())
        r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
