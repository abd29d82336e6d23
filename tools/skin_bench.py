#!/usr/bin/env python
"""The deformation tick with the skinning on the device, beside the tick that skins on the host: tools/deform_bench.py's protocol
on scenedefs.skinned_room -- 1080p, 1 spp, 5 bounces, 3 frames in flight, 4 warm-up ticks, 30 timed -- at three mesh sizes.

  (a) host         the skinned vertices arrive as host arrays (the skinning itself is NOT timed: a CPU step the caller owns):
                   atn_update_geometry -> atn_lbvh_rebuild_list -> atn_update_tlas -> atn_render
  (b) device       atn_skin_update -> atn_skin_compute returning the box (the reference's read-back) -> atn_lbvh_rebuild_list
                   -> atn_update_tlas -> atn_render
  (c) no read-back atn_skin_update -> atn_skin_compute(NULL, NULL) -> atn_lbvh_rebuild_list_skinned -> atn_update_tlas -> atn_render

ms per tick-and-frame: a host clock around `--ticks` ticks that end in a device synchronise, `--repeats` windows per path, the paths
taken in turn inside one process (a, b, c, a, b, c, ...); median, min and max of the windows.  Per step: the median over 12 calls of
the call alone (`call`: what the host thread pays) and of the call followed by a synchronise (`done`: until the device has finished
it), frames idle.  The top layer handed to atn_update_tlas is ONE conservative top layer for every tick and every path (the box of
all poses): the bench measures the tick, tests/test_gpu_skinning.py the films.  All three paths upload the same poses; (a)'s host
arrays are what the device path computed for them (equal to the CPU twin's, bit for bit).

    python tools/skin_bench.py [--sizes 48x24,160x80,448x224] [--ticks 30] [--warmup 4] [--repeats 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_BONES = 24
N_POSES = 6
W, H = 1920, 1080


def one_size(nu, nv, args):
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    b, oid, cam, sv = scenedefs.skinned_room(nu, nv, N_BONES)
    fs0 = b.build()
    o = fs0.arrays["objects"][oid]
    t0, n = int(o["triangle_id"]), int(o["triangle_num"])
    tris0 = fs0.arrays["triangles"][t0:t0 + n]
    v0, v1 = int(tris0["idx"].min()), int(tris0["idx"].max()) + 1
    lst = fs0.blas_index[oid]
    poses = [scenedefs.skinned_pose(0.4 * k, N_BONES) for k in range(N_POSES)]

    r = PathTracing(0)
    r.UpdateSceneData(fs0)
    r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H))
    r.initSampler(W, H, 0)
    skin = r.skin_create(sv, v0, t0, n, N_BONES)
    # the poses as a host skinning step would hand them over, and the box of all of them
    host = []
    for k, pal in enumerate(poses):
        r.skin_update(skin, pal)
        mn, mx = r.skin_compute(skin, k == 0)
        tr = tris0.copy()
        tr["area"] = r.skin_buffer(skin, "area")
        host.append(dict(pos=r.skin_buffer(skin, "pos").copy(), nml=r.skin_buffer(skin, "nml").copy(), tris=tr, bmin=mn.copy(), bmax=mx.copy()))
    lo, hi = np.min([h["bmin"] for h in host], 0), np.max([h["bmax"] for h in host], 0)
    b.pos[v0] = (float(lo[0]), float(lo[1]), float(lo[2]), b.pos[v0][3])
    b.pos[v0 + 1] = (float(hi[0]), float(hi[1]), float(hi[2]), b.pos[v0 + 1][3])
    top = b.build()                                  # its top layer holds the tube's instance under the box of all poses
    r.UpdateSceneData(fs0)                           # a clean scene (and a new skin: the old one died with the upload)
    skin = r.skin_create(sv, v0, t0, n, N_BONES)
    r.set_frames_in_flight(3)

    def geom(i):
        h = host[i % N_POSES]
        r.updateGeometry(vtx_pos=h["pos"], vtx_nml=h["nml"], vtx_offset=v0, triangles=h["tris"], tri_offset=t0)

    def lbvh_host(i):
        h = host[i % N_POSES]
        r.lbvh_rebuild_list(lst, t0, n, h["bmin"], h["bmax"])

    box = [None]

    def skin_update(i):
        r.skin_update(skin, poses[i % N_POSES])

    def compute_box(i):
        box[0] = r.skin_compute(skin, i == 0)

    def lbvh_box(i):
        r.lbvh_rebuild_list(lst, t0, n, box[0][0], box[0][1])

    def compute_nobox(i):
        r.skin_compute(skin, i == 0, want_bbox=False)

    def lbvh_skinned(i):
        r.lbvh_rebuild_list_skinned(lst, skin)

    def tlas(i):
        r.updateBVH(top)

    paths = {
        "a_host": [("update_geometry", geom), ("lbvh_rebuild", lbvh_host), ("update_tlas", tlas)],
        "b_device_readback": [("skin_update", skin_update), ("skin_compute", compute_box), ("lbvh_rebuild", lbvh_box), ("update_tlas", tlas)],
        "c_device_no_readback": [("skin_update", skin_update), ("skin_compute", compute_nobox), ("lbvh_rebuild_skinned", lbvh_skinned), ("update_tlas", tlas)],
    }

    def tick(steps, i):
        for _, f in steps:
            f(i)
        r.render(W, H, 5, 3, frame=i, download=False)

    windows = {k: [] for k in paths}
    for name, steps in paths.items():
        for i in range(args.warmup):
            tick(steps, i)
        r.synchronize()
    for _ in range(args.repeats):
        for name, steps in paths.items():
            tick(steps, 0)                           # the path's own geometry in every copy of the scene before its window
            r.synchronize()
            t = time.perf_counter()
            for i in range(args.ticks):
                tick(steps, i)
            r.synchronize()
            windows[name].append((time.perf_counter() - t) / args.ticks * 1e3)
    res = dict(triangles=n, vertices=v1 - v0, bones=N_BONES, paths={})
    for name, steps in paths.items():
        per = {}
        compute_box(0)                               # (lbvh_box needs a box whatever ran last)
        for sname, f in steps:
            call, done = [], []
            for i in range(12):
                r.synchronize()
                t = time.perf_counter()
                f(i)
                call.append((time.perf_counter() - t) * 1e3)
                r.synchronize()
                done.append((time.perf_counter() - t) * 1e3)
            per[sname] = dict(call_ms=round(float(np.median(call)), 4), done_ms=round(float(np.median(done)), 4))
        w = windows[name]
        res["paths"][name] = dict(ms_per_tick_and_frame=dict(median=round(float(np.median(w)), 4), min=round(min(w), 4), max=round(max(w), 4)),
                                  steps=per)
    t = time.perf_counter()
    for i in range(args.ticks):
        r.render(W, H, 5, 3, frame=i, download=False)
    r.synchronize()
    res["ms_per_frame_static"] = round((time.perf_counter() - t) / args.ticks * 1e3, 4)
    res["upload_bytes_per_tick"] = dict(a_host=2 * 16 * (v1 - v0) + 32 * n, b_device_readback=64 * N_BONES, c_device_no_readback=64 * N_BONES)
    res["shade_records_repacked_per_tick"] = dict(a_host=len(fs0.arrays["triangles"]) + n, b_device_readback=2 * n, c_device_no_readback=n)
    r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="48x24,160x80,448x224")
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = dict(workload="skinned_room (Cornell box + skinned tube, %d bones), %dx%d 1 spp 5 bounces, 3 frames in flight" % (N_BONES, W, H),
               protocol="%d warm-up ticks, %d timed per window, %d windows per path taken in turn in one process" % (args.warmup, args.ticks, args.repeats),
               sizes=[])
    for s in args.sizes.split(","):
        nu, nv = (int(x) for x in s.split("x"))
        res = one_size(nu, nv, args)
        out["sizes"].append(res)
        print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
