#!/usr/bin/env python
"""The top layer built on the device (atn_tlas_rebuild, docs/TLAS.md) beside the host-built one, for 8 instances (the atrium), 1 024
and 16 384 (a jittered grid of one icosphere mesh): tools/mgpu_svgf_bench.py's window protocol -- the configurations taken in turn
inside one process, `--repeats` windows each, median (min .. max).

  (a) host time per tick [ms, host clock, nothing waited for inside the window]
        host    atns_build_tlas over the instances' world boxes + atn_update_tlas   (the boxes themselves come precomputed: a
                caller has them from its own transforms; numpy's time for them is reported apart, as boxes_numpy)
        device  atn_tlas_rebuild with the same objects and matrices
      and the skinned tick of skinned_room: skin_update -> skin_compute -> list rebuild -> top layer,
        readback   the box returned by skin_compute, atns_build_tlas from it, atn_update_tlas
        device     nothing read back: atn_lbvh_rebuild_list_skinned, atn_tlas_rebuild()
  (b) GPU time of the rebuild [ms]: a HIP event pair on the update stream (one frame in flight: the context's main stream) around
      atn_tlas_rebuild() without arguments -- the kernels alone -- block path against the forced general path at 8 and 1 024
  (c) ms per frame through the device-built layer against the host SAH layer: same scene, same matrices, two contexts taken in turn

    python tools/tlas_bench.py [--ticks 50] [--frames 20] [--warmup 3] [--repeats 5] [--sizes 8,1024,16384] [--out profiles/tlas_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H = 1280, 720


def instance_boxes(fs):
    """World boxes of fs's instances from the lists' roots through the current L2W matrices (SceneBuilder.build's arithmetic,
    vectorised): (boxes float32 [n, 6], object ids, list ids)."""
    from aten_amd import layout as L
    a = fs.arrays
    oids = np.array([i for i, o in enumerate(a["objects"]) if o["type"] == L.OBJ_INSTANCE], np.int32)
    exids = np.array([fs.blas_index[int(a["objects"][i]["object_id"])] for i in oids], np.int32)
    roots = np.array([[*a["bvh_lists"][e][0]["boxmin"], *a["bvh_lists"][e][0]["boxmax"]] for e in exids], np.float32)
    return roots, oids, exids


def world_boxes(roots, mtx):
    sel = np.array([[(c >> k) & 1 for k in range(3)] for c in range(8)])
    corners = np.stack([roots[:, 3 * sel[:, k] + k] for k in range(3)], -1)                 # [n, 8, 3]
    w = np.einsum("nij,nkj->nki", mtx[:, :3, :3], corners) + mtx[:, None, :3, 3]
    return np.concatenate([w.min(1), w.max(1)], 1).astype(np.float32)


def host_top(boxes, oids, exids):
    from aten_amd import layout as L
    from aten_amd._hostlib import hostlib
    lib = hostlib()
    mesh_ids = np.full(len(oids), -1, np.int32)
    out = C.c_void_p(); cnt = C.c_uint32()
    rc = lib.atns_build_tlas(L.ptr(boxes), L.ptr(oids), L.ptr(exids), L.ptr(mesh_ids), len(oids), C.byref(out), C.byref(cnt))
    assert rc == 0
    top = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(cnt.value * 48,)).view(L.BVH_NODE).copy()
    lib.atns_free(out)
    return top


def grid_scene(n):
    """n instances of one icosphere (80 triangles) on a jittered square grid, each with a rigid matrix; a sky-lit diffuse scene."""
    from aten_amd import layout as L
    from aten_amd.scene import scenedefs
    from aten_amd.scene.builder import SceneBuilder
    b = SceneBuilder()
    m = b.add_material("ball", L.MTRL_DIFFUSE, (0.7, 0.6, 0.5))
    v, f = scenedefs._icosphere(1)
    oid = b.add_mesh("ball", np.asarray(v, np.float32) * 0.4, np.asarray(f, np.int64), m, normals=np.asarray(v, np.float32))
    side = int(np.ceil(np.sqrt(n)))
    inst = [b.create_instance(oid, np.eye(4, dtype=np.float32)) for _ in range(n)]
    b.set_background((0.6, 0.7, 0.9))
    fs = b.build()
    cam = dict(pos=(0.0, 0.35 * side, 0.75 * side), at=(0.0, 0.0, 0.0), vfov=45.0)
    return fs, cam, inst, side


def grid_matrices(fs, inst, side, phase):
    rng = np.random.default_rng(1)
    n = len(inst)
    mtx = fs.arrays["matrices"].copy()
    ids = fs.arrays["objects"]["mtx_id"][inst]
    gx, gz = np.arange(n) % side - 0.5 * side, np.arange(n) // side - 0.5 * side
    ang = rng.uniform(0, 6.28, n) + phase
    c, s = np.cos(ang), np.sin(ang)
    M = np.tile(np.eye(4), (n, 1, 1))
    M[:, 0, 0], M[:, 0, 2], M[:, 2, 0], M[:, 2, 2] = c, s, -s, c
    M[:, 0, 3] = gx + rng.uniform(-0.2, 0.2, n) + 0.1 * np.sin(phase)
    M[:, 1, 3] = rng.uniform(0.0, 0.6, n)
    M[:, 2, 3] = gz + rng.uniform(-0.2, 0.2, n)
    mtx[ids] = M.astype(np.float32)
    mtx[ids + 1] = np.linalg.inv(M).astype(np.float32)
    return mtx


def atrium_matrices(fs, phase):
    """The atrium's instances that have a matrix turn about y by `phase` on top of their placement."""
    mtx = fs.arrays["matrices"].copy()
    c, s = np.cos(phase), np.sin(phase)
    R = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    for k in range(0, len(mtx), 2):
        if not np.array_equal(mtx[k], np.eye(4, dtype=np.float32)):
            M = mtx[k].astype(np.float64) @ R
            mtx[k] = M.astype(np.float32); mtx[k + 1] = np.linalg.inv(M).astype(np.float32)
    return mtx


def stats(w):
    return dict(median=round(float(np.median(w)), 4), min=round(float(min(w)), 4), max=round(float(max(w)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="8,1024,16384")
    ap.add_argument("--out", default=os.path.join("profiles", "tlas_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tlas_bench: no GPU (there is nothing to measure without one)")
    torch.cuda.init()
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    result = dict(protocol="%d ticks / %d frames per window after %d warm-up, %d windows per configuration taken in turn in one process; %dx%d frames, 1 spp, 5 bounces"
                           % (args.ticks, args.frames, args.warmup, args.repeats, W, H),
                  device=torch.cuda.get_device_name(0), host_tick_ms={}, rebuild_gpu_ms={}, frame_ms={})

    def context(fs, cam):
        r = PathTracing(0)
        r.UpdateSceneData(fs); r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)); r.initSampler(W, H, 0)
        return r

    for n in [int(x) for x in args.sizes.split(",")]:
        if n == 8:
            fs, cam = scenedefs.atrium()
            phases = [atrium_matrices(fs, 0.1 * k) for k in range(4)]
        else:
            fs, cam, inst, side = grid_scene(n)
            phases = [grid_matrices(fs, inst, side, 0.3 * k) for k in range(4)]
        name = "%d instances" % len([o for o in fs.arrays["objects"] if o["type"] == 1])
        objs = np.ascontiguousarray(fs.arrays["objects"])
        roots, oids, exids = instance_boxes(fs)
        mids = objs["mtx_id"][oids]
        t = time.perf_counter()
        boxes = [world_boxes(roots, np.where((mids >= 0)[:, None, None], m[np.maximum(mids, 0)], np.eye(4, dtype=np.float32))) for m in phases]
        boxes_ms = (time.perf_counter() - t) / len(phases) * 1e3
        host, dev = context(fs, cam), context(fs, cam)
        l = host._l

        def host_tick(k):
            top = host_top(boxes[k % 4], oids, exids)
            m = phases[k % 4]
            host._check(l.atn_update_tlas(host._ctx, objs.ctypes.data, len(objs), m.ctypes.data, len(m), top.ctypes.data, len(top)))

        def dev_tick(k, general=False):
            dev.tlas_rebuild(objs, phases[k % 4], force_general=general)

        # (a) host time per tick
        win = {"host": [], "device": []}
        for k in range(args.warmup):
            host_tick(k); dev_tick(k)
        for _ in range(args.repeats):
            for key, r, f in (("host", host, host_tick), ("device", dev, dev_tick)):
                r.synchronize()
                t = time.perf_counter()
                for k in range(args.ticks):
                    f(k)
                win[key].append((time.perf_counter() - t) / args.ticks * 1e3)
                r.synchronize()
        result["host_tick_ms"][name] = dict(host=stats(win["host"]), device=stats(win["device"]), boxes_numpy=round(boxes_ms, 4))

        # (b) GPU time of the rebuild's kernels
        if n <= 1024:
            s = torch.cuda.ExternalStream(dev.stream_ptr())
            ev = {"block": [], "general": []}
            for rep in range(args.repeats * 4 + 2):
                for key in ("block", "general"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    dev.tlas_rebuild(force_general=(key == "general"))
                    e1.record(s)
                    e1.synchronize()
                    if rep >= 2:
                        ev[key].append(e0.elapsed_time(e1))
            result["rebuild_gpu_ms"][name] = {k: stats(v) for k, v in ev.items()}

        # (c) ms per frame through either layer, the same matrices in both contexts
        host_tick(1); dev_tick(1)
        win = {"host_sah_layer": [], "device_lbvh_layer": []}
        frame = 0
        for _ in range(args.warmup):
            host.render(W, H, frame=frame, download=False); dev.render(W, H, frame=frame, download=False); frame += 1
        for _ in range(args.repeats):
            for key, r in (("host_sah_layer", host), ("device_lbvh_layer", dev)):
                r.synchronize()
                t = time.perf_counter()
                for k in range(args.frames):
                    r.render(W, H, frame=frame + k, download=False)
                r.synchronize()
                win[key].append((time.perf_counter() - t) / args.frames * 1e3)
            frame += args.frames
        result["frame_ms"][name] = {k: stats(v) for k, v in win.items()}
        host.close(); dev.close()

    # the skinned tick, with and without the box read-back
    b, oid, cam, sv = scenedefs.skinned_room()
    fs = b.build()
    o = fs.arrays["objects"][oid]
    t0, nt = int(o["triangle_id"]), int(o["triangle_num"])
    v0 = int(fs.arrays["triangles"][t0:t0 + nt]["idx"].min())
    lst = fs.blas_index[oid]
    objs = np.ascontiguousarray(fs.arrays["objects"]); mtx = np.ascontiguousarray(fs.arrays["matrices"])
    roots, oids, exids = instance_boxes(fs)
    tube = int(np.nonzero(exids == lst)[0][0])
    pal = [scenedefs.skinned_pose(0.4 + 0.3 * k, 8) for k in range(4)]
    back, dev = context(fs, cam), context(fs, cam)
    skins = [x.skin_create(sv, v0, t0, nt, 8) for x in (back, dev)]

    def back_tick(k):
        back.skin_update(skins[0], pal[k % 4])
        mn, mx = back.skin_compute(skins[0], k == 0)
        back.lbvh_rebuild_list(lst, t0, nt, mn, mx)
        boxes = roots.copy(); boxes[tube] = np.concatenate([mn, mx])       # (every instance of the room has the identity matrix)
        top = host_top(boxes, oids, exids)
        back._check(back._l.atn_update_tlas(back._ctx, objs.ctypes.data, len(objs), mtx.ctypes.data, len(mtx), top.ctypes.data, len(top)))

    def dev_tick(k):
        dev.skin_update(skins[1], pal[k % 4])
        dev.skin_compute(skins[1], k == 0, want_bbox=False)
        dev.lbvh_rebuild_list_skinned(lst, skins[1])
        dev.tlas_rebuild()
    win = {"readback": [], "device": []}
    for k in range(args.warmup):
        back_tick(k); dev_tick(k)
    for _ in range(args.repeats):
        for key, r, f in (("readback", back, back_tick), ("device", dev, dev_tick)):
            r.synchronize()
            t = time.perf_counter()
            for k in range(1, args.ticks + 1):
                f(k)
            win[key].append((time.perf_counter() - t) / args.ticks * 1e3)
            r.synchronize()
    result["host_tick_ms"]["skinned_room tick"] = {k: stats(v) for k, v in win.items()}
    back.close(); dev.close()

    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
