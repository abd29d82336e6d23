#!/usr/bin/env python
"""Volume frame cost (atn_volume_render) on fog_sponza (sponza_lod with a slab of thin fog) and cornell_box_smoke, 1080p, 1 spp,
maxDepth 5, one frame in flight, beside atn_render on the same scene without its medium box (sponza_lod, cornell_box).  Prints one
JSON line.

ms per frame: device events (torch.cuda.Event on the context's own stream) around `--steps` frames after `--warmup`, repeated
`--repeats` times (median and spread).  Per kernel kind: the library's own event spans over `--steps` profiled frames (gen, closest =
k_vol_closest, shade = k_vol_shade, trace_fused = k_vol_transmit, gather).  Segments per connection: the frame counters of
atn_volume_download(4).  `--scenes smoke_grid_sponza` (fog_sponza with the fog replaced by a 64^3 procedural grid) measures grid
media: its grids are set with volume_set_grids, and the cap counters of atn_volume_download(5) are reported.

    python tools/volume_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--width 1920 --height 1080]
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
    ap.add_argument("--scenes", default="fog_sponza,cornell_box_smoke")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    W, H = args.width, args.height
    plain = {"fog_sponza": "sponza_lod", "cornell_box_smoke": "cornell_box", "smoke_grid_sponza": "sponza_lod", "cornell_box_smoke_grid": "cornell_box"}
    res = {"metric": "ms per frame (%dx%d, 1 spp, maxDepth %d, 1 frame in flight)" % (W, H, args.depth),
           "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "cases": {}}

    def bench(scene_name, volume):
        fs, cam = getattr(scenedefs, scene_name)()
        r = PathTracing(0)
        r.UpdateSceneData(fs)
        r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H))
        r.initSampler(W, H, 0)
        if volume and fs.grids:
            r.volume_set_grids(fs.grids)
        r._l.atn_stream.restype = C.c_void_p
        stream = torch.cuda.ExternalStream(r._l.atn_stream(r._ctx))
        frame = [0]

        def step(profile=False):
            (r.volume_render if volume else r.render)(W, H, max_depth=args.depth, frame=frame[0], download=False, profile=profile)
            frame[0] += 1
        for _ in range(args.warmup):
            step()
        ms = []
        for _ in range(args.repeats):
            r._l.atn_synchronize(r._ctx)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                step()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        out = {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
               "mrays_per_s": round(W * H / 1e6 / (float(np.median(ms)) / 1e3), 3)}
        r.reset_kernel_times()
        for _ in range(args.steps):
            step(profile=True)
        r._l.atn_synchronize(r._ctx)
        out["kernel_ms_per_frame"] = {k: round(ms_ / args.steps, 4) for k, (ms_, n_) in r.kernel_times().items() if n_}
        if volume:
            cnt = r.volume_buffer("counters")
            out["counters_last_frame"] = cnt
            out["segments_per_connection"] = round(cnt["segments"] / max(cnt["connections"], 1), 4)
            if fs.grids:
                out["grid_counters_last_frame"] = r.volume_buffer("grid_counters")
        r.close()
        return out
    for name in args.scenes.split(","):
        res["cases"][name + "/volume"] = bench(name, True)
        res["cases"][plain[name] + "/path_tracer"] = bench(plain[name], False)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
