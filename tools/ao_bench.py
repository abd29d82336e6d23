#!/usr/bin/env python
"""AO frame cost (atn_ao_render) on sponza_lod, 1080p, one frame in flight, break_on_terminate = 0 (every pixel written), beside
atn_render at maxDepth = 1 on the same scene.  Cases: num_rays 1 and 8, the radius at 1.0 and at a tenth of the scene's diagonal, and
the filter on at (8, 1.0).  Prints one JSON line and writes it to --out.

ms per frame: device events (torch.cuda.Event on the context's own stream) around `--steps` frames after `--warmup`, repeated
`--repeats` times (median and spread).  Per-kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ao_bench.py --steps 5 --warmup 1 --repeats 1 --out /dev/null

    python tools/ao_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--width 1920 --height 1080] [--out profiles/ao_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ao_bench.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    W, H = args.width, args.height
    fs, cam = scenedefs.sponza_lod()
    pos = fs.arrays["vtx_pos"][:, :3]
    diagonal = float(np.linalg.norm(pos.max(0).astype(np.float64) - pos.min(0).astype(np.float64)))
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

    def ao_step():
        r.ao_render(W, H, frame=frame[0], break_on_terminate=False, download=False)
        frame[0] += 1

    def pt_step():
        r.render(W, H, max_depth=1, frame=frame[0], download=False)
        frame[0] += 1

    res = {"metric": "ms per AO frame (sponza_lod, %dx%d, 1 frame in flight, break_on_terminate 0)" % (W, H),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "scene_diagonal": round(diagonal, 4), "cases": {}}

    def record(name, step, rays):
        r.ao_reset()
        frame[0] = 0
        ms = timed(step)
        med = float(np.median(ms))
        res["cases"][name] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                              "mrays_per_s": round(W * H * rays / 1e6 / (med / 1e3), 3)}

    for num_rays in (1, 8):
        for rname, radius in (("1.0", 1.0), ("diagonal/10", diagonal / 10.0)):
            r.ao_set_params(num_rays, radius, False)
            record("ao rays %d radius %s" % (num_rays, rname), ao_step, 1 + num_rays)
    r.ao_set_params(8, 1.0, True)
    record("ao rays 8 radius 1.0 filter", ao_step, 9)
    record("path_tracer maxDepth 1", pt_step, 1)
    r.close()
    line = json.dumps(res)
    print(line)
    if args.out and args.out != "/dev/null":
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
