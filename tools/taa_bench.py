#!/usr/bin/env python
"""What the display tail (atn_taa_resolve: TAA + history write + gamma / RGBA8, one launch; docs/TAA.md) adds to an SVGF frame:
tools/skin_bench.py's window protocol on BASELINE config 5's shape -- sponza_lod, 1080p, 1 spp, 5 bounces, SVGF frames with
compute_motion = 1, 3 frames in flight.

  (a) svgf         atn_svgf_render per frame                      (the yardstick: the same frame as without this tool, same process)
  (b) svgf_taa     atn_svgf_render + atn_taa_resolve(source 0) per frame, no host wait in between

ms per frame: a host clock around `--frames` frames that end in a device synchronise, `--repeats` windows per path, the paths taken in
turn inside one process (a, b, a, b, ...); median, min and max of the windows.  The kernel alone: `--launches` atn_taa_resolve calls
on the last frame enqueued back to back on an otherwise idle device, one synchronise at the end, / launches (the history advances with
every call; the traffic per call is the same).  Beside it the compulsory traffic: three float4 planes read, one float4 and one RGBA8
plane written = 68 bytes per pixel.

    python tools/taa_bench.py [--frames 30] [--warmup 4] [--repeats 5] [--launches 200] [--frames-in-flight 3] [--out profiles/taa_bench.json]
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
BYTES_PER_PIXEL = 3 * 16 + 16 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames-in-flight", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "taa_bench.json"))
    args = ap.parse_args()
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    fs, cam = scenedefs.sponza_lod()
    r = PathTracing(0)
    r.UpdateSceneData(fs)
    r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H))
    r.initSampler(W, H, 0)
    r.set_frames_in_flight(args.frames_in_flight)
    frame = [0]

    def svgf():
        r.svgf_render(W, H, DEPTH, RR, frame=frame[0], compute_motion=1, download=False)
        frame[0] += 1

    def svgf_taa():
        svgf()
        r.taa_resolve(W, H, "svgf")

    paths = {"a_svgf": svgf, "b_svgf_taa": svgf_taa}
    windows = {k: [] for k in paths}
    for f in paths.values():
        for _ in range(args.warmup):
            f()
        r.synchronize()
    for _ in range(args.repeats):
        for name, f in paths.items():
            f()
            r.synchronize()
            t = time.perf_counter()
            for _ in range(args.frames):
                f()
            r.synchronize()
            windows[name].append((time.perf_counter() - t) / args.frames * 1e3)
    # the kernel alone, frames idle
    kernel = []
    for _ in range(args.repeats):
        r.taa_resolve(W, H, "svgf")
        r.synchronize()
        t = time.perf_counter()
        for _ in range(args.launches):
            r.taa_resolve(W, H, "svgf")
        r.synchronize()
        kernel.append((time.perf_counter() - t) / args.launches * 1e3)
    r.close()

    def stats(w):
        return dict(median=round(float(np.median(w)), 4), min=round(min(w), 4), max=round(max(w), 4))
    traffic_mb = BYTES_PER_PIXEL * W * H / 1e6
    k = float(np.median(kernel))
    out = dict(workload="sponza_lod %dx%d 1 spp %d bounces, SVGF frames (compute_motion = 1), %d frames in flight" % (W, H, DEPTH, args.frames_in_flight),
               protocol="%d warm-up frames, %d timed per window, %d windows per path taken in turn in one process; kernel: %d launches back to back on an idle device"
                        % (args.warmup, args.frames, args.repeats, args.launches),
               ms_per_frame={n: stats(w) for n, w in windows.items()},
               taa_added_ms_per_frame=round(float(np.median(windows["b_svgf_taa"]) - np.median(windows["a_svgf"])), 4),
               kernel_ms=stats(kernel),
               compulsory_traffic=dict(bytes_per_pixel=BYTES_PER_PIXEL, megabytes_per_frame=round(traffic_mb, 1),
                                       gigabytes_per_second_at_kernel_ms=round(traffic_mb / k, 1) if k > 0 else None))
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
