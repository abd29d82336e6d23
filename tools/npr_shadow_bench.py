#!/usr/bin/env python
"""Cost of the NPR shadow pre-pass (atn_npr_shadow_set_mode(1); docs/NPR_SHADOW.md): atn_render in mode 0 against mode 1 on
stylized_shadow_room and stylized_shadow_sponza, 1080p, 1 spp, 5 bounces, with one frame in flight and with four.  Prints one JSON
line.

ms per frame: device events (torch.cuda.Event on the context's own stream) around `--steps` frames after `--warmup`, repeated
`--repeats` times (median and spread); with frames in flight the events bracket the whole batch of frames and the context is
synchronised before the second one is read.  `--only SCENE:MODE:IN_FLIGHT` runs one case alone (for a kernel trace of its own:
rocprofv3 --kernel-trace --stats -- python tools/npr_shadow_bench.py --only sponza:1:1 --repeats 1).

    python tools/npr_shadow_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--width 1920 --height 1080] [--only room:1:1]
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
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    W, H = args.width, args.height
    scenes = {"room": scenedefs.stylized_shadow_room, "sponza": scenedefs.stylized_shadow_sponza}
    cases = [(s, m, n) for s in scenes for n in (1, 4) for m in (0, 1)]
    if args.only:
        s, m, n = args.only.split(":")
        cases = [(s, int(m), int(n))]
    res = {"metric": "ms per atn_render frame (%dx%d, 1 spp, %d bounces), NPR shadow mode 0 / 1" % (W, H, args.depth),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    built = {}
    for name, mode, in_flight in cases:
        if name not in built:
            built[name] = scenes[name]()
        fs, cam = built[name]
        r = PathTracing(0)
        try:
            r.UpdateSceneData(fs)
            r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H))
            r.initSampler(W, H, 0)
            r.set_frames_in_flight(in_flight)
            r.set_npr_shadow(mode)
            r._l.atn_stream.restype = C.c_void_p
            frame = [0]

            def step():
                r.render(W, H, max_depth=args.depth, frame=frame[0], download=False)
                frame[0] += 1

            for _ in range(args.warmup):
                step()
            ms = []
            for _ in range(args.repeats):
                r.synchronize()
                # (the current bank's stream: the first frame of the batch is enqueued behind e0, and after synchronize() every
                # bank is idle, so e1 on the last frame's stream -- read after another synchronize() -- closes the batch)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(torch.cuda.ExternalStream(r._l.atn_stream(r._ctx)))
                for _ in range(args.steps):
                    step()
                r.synchronize()
                e1.record(torch.cuda.ExternalStream(r._l.atn_stream(r._ctx)))
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / args.steps)
            res["cases"]["%s mode %d, %d in flight" % (name, mode, in_flight)] = {
                "ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
        finally:
            r.close()
    for name in scenes:
        for n in (1, 4):
            a, b = res["cases"].get("%s mode 0, %d in flight" % (name, n)), res["cases"].get("%s mode 1, %d in flight" % (name, n))
            if a and b:
                res["cases"]["%s pre-pass, %d in flight" % (name, n)] = {
                    "ms": round(b["ms_median"] - a["ms_median"], 4), "share_of_mode_1_frame": round(1.0 - a["ms_median"] / b["ms_median"], 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
