#!/usr/bin/env python
"""What testing sphere leaves costs a frame (atn_set_sphere_intersection, docs/SPHERES.md): sponza_lod plus two spheres
(tests/sphere_cases.py: spheres_sponza), 1080p, 1 spp, 5 bounces, one frame in flight -- mode 1 (the sphere-aware kernels of
spheres.hip) against mode 0 (the same scene, its spheres dead leaves).  Prints one JSON line and writes it to --out.

ms per frame: device events (torch.cuda.Event on the context's own stream) around `--steps` frames after `--warmup`, repeated
`--repeats` times (median and spread).  The two modes do not render the same image -- in mode 1 the spheres are there -- so the
number is the cost of the feature in use, not of a code path alone.

    python tools/sphere_bench.py [--steps 30] [--warmup 5] [--repeats 5] [--width 1920 --height 1080] [--out profiles/sphere_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sphere_bench.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import sphere_cases as SC
    from aten_amd.renderer import PathTracing
    from aten_amd.scene.camera import create_camera
    W, H = args.width, args.height
    fs, cam = SC.spheres_sponza()
    c = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)
    res = {"metric": "ms per frame (spheres_sponza, %dx%d, 1 spp, 5 bounces, 1 frame in flight)" % (W, H),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}
    for mode in (0, 1, 0, 1):
        r = PathTracing(0)
        r.set_sphere_intersection(mode)
        r.UpdateSceneData(fs)
        r.updateCamera(c)
        r.initSampler(W, H, 0)
        r._l.atn_stream.restype = C.c_void_p
        stream = torch.cuda.ExternalStream(r._l.atn_stream(r._ctx))
        frame = 0
        for _ in range(args.warmup):
            r.render(W, H, 5, 3, frame=frame, download=False); frame += 1
        ms = []
        for _ in range(args.repeats):
            r._l.atn_synchronize(r._ctx)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                r.render(W, H, 5, 3, frame=frame, download=False); frame += 1
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        name = "mode %d" % mode
        res["cases"].setdefault(name, []).append({"sphere_leaves": r.sphere_leaves(), "ms_median": round(float(np.median(ms)), 4),
                                                  "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)})
        r.close()
    m0 = float(np.median([x["ms_median"] for x in res["cases"]["mode 0"]]))
    m1 = float(np.median([x["ms_median"] for x in res["cases"]["mode 1"]]))
    res["mode1_over_mode0"] = round(m1 / m0, 4)
    line = json.dumps(res)
    print(line)
    if args.out and args.out != "/dev/null":
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
