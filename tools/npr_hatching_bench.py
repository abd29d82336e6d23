#!/usr/bin/env python
"""Cost of the NPR hatching pre-pass per (base, direction) cell (atn_npr_hatching_set; docs/NPR_HATCHING.md): atn_render in mode 0
against mode 1 with every setting on stylized_shadow_room and stylized_shadow_sponza, 1080p, 1 spp, 5 bounces, with one frame in
flight and with four.  Prints one JSON line.

ms per frame as tools/npr_shadow_bench.py measures it: device events (torch.cuda.Event on the context's own stream) around `--steps`
frames after `--warmup`, repeated `--repeats` times (median and spread).  One context per (scene, frames in flight); the settings are
switched between the cells and every cell warms up again.  `--only SCENE:IN_FLIGHT` runs one context alone, `--cells` a list of
BASE:DIRECTION:RAYS cells (`0` alone: mode 0) -- for a kernel trace of its own:
rocprofv3 --kernel-trace --stats -- python tools/npr_hatching_bench.py --only room:1 --cells 1:4:1,1:1:1,1:2:1 --repeats 1

    python tools/npr_hatching_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--width 1920 --height 1080] [--only room:1] [--cells ...]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIRECTIONS = ("none", "horizontal", "vertical", "orthogonal", "cross", "orthogonal_cross")


def cell_name(cell):
    if cell is None:
        return "mode 0"
    base, direction, rays = cell
    return "shadow_ray %s" % DIRECTIONS[direction] if base == 1 else "ao[%d] %s" % (rays, DIRECTIONS[direction])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--cells", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    W, H = args.width, args.height
    scenes = {"room": scenedefs.stylized_shadow_room, "sponza": scenedefs.stylized_shadow_sponza}
    contexts = [(s, n) for s in scenes for n in (1, 4)]
    if args.only:
        s, n = args.only.split(":")
        contexts = [(s, int(n))]
    cells = [None] + [(1, d, 1) for d in range(6)] + [(0, d, rays) for rays in (1, 4) for d in range(6)]
    if args.cells:
        cells = [None if c == "0" else tuple(int(v) for v in c.split(":")) for c in args.cells.split(",")]
    res = {"metric": "ms per atn_render frame (%dx%d, 1 spp, %d bounces) per NPR hatching cell; pre-pass = the cell - mode 0" % (W, H, args.depth),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    built = {}
    for name, in_flight in contexts:
        if name not in built:
            built[name] = scenes[name]()
        fs, cam = built[name]
        r = PathTracing(0)
        try:
            r.UpdateSceneData(fs)
            r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H))
            r.initSampler(W, H, 0)
            r.set_frames_in_flight(in_flight)
            r._l.atn_stream.restype = C.c_void_p
            frame = [0]

            def step():
                r.render(W, H, max_depth=args.depth, frame=frame[0], download=False)
                frame[0] += 1

            for cell in cells:
                r.set_npr_shadow(0 if cell is None else 1)
                if cell is not None:
                    r.set_npr_hatching(cell[0], cell[1], cell[2], 1.0)
                for _ in range(args.warmup):
                    step()
                ms = []
                for _ in range(args.repeats):
                    r.synchronize()
                    # (as tools/npr_shadow_bench.py: e0 on the current bank's stream in front of the batch, e1 behind a synchronize())
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(torch.cuda.ExternalStream(r._l.atn_stream(r._ctx)))
                    for _ in range(args.steps):
                        step()
                    r.synchronize()
                    e1.record(torch.cuda.ExternalStream(r._l.atn_stream(r._ctx)))
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1) / args.steps)
                res["cases"]["%s, %d in flight: %s" % (name, in_flight, cell_name(cell))] = {
                    "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
        finally:
            r.close()
        zero = res["cases"].get("%s, %d in flight: mode 0" % (name, in_flight))
        if zero:
            for cell in cells:
                if cell is not None:
                    c = res["cases"]["%s, %d in flight: %s" % (name, in_flight, cell_name(cell))]
                    c["prepass_ms"] = round(c["ms_median"] - zero["ms_median"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
