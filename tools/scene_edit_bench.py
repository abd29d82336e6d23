#!/usr/bin/env python
"""What a scene edit costs beside the only other way to make the same change, a re-upload (docs/SCENE_EDITS.md).

On sponza_lod and the atrium: the wall time of atn_update_materials (one material / the whole array), atn_update_lights,
atn_update_texture (one 256 x 256 texture uploaded beside the scene's own) and atn_update_rendering_config, and of atn_upload_scene of
the same scene.  Every call is synchronous (it returns when the device holds the change), frames idle; one warm-up call, then the
median of `--repeats` calls, in ms.  Each scene is measured in a child process of its own under a time limit (a fault or a hang in
one ends that child, and nothing more is started on the GPU); the parent prints ONE JSON line.

    python tools/scene_edit_bench.py [--scenes sponza_lod,atrium] [--repeats 5] [--timeout 300] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TEX = 256


def median_ms(f, repeats):
    f()                                             # warm-up
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4)


def one_scene(name, repeats):
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    rng = np.random.default_rng(3)
    extra = {}

    def add_texture(b, *_):
        extra["tex"] = b.add_texture("edit_bench_%d" % TEX, rng.random((TEX, TEX, 4)).astype(np.float32))
    if name == "sponza_lod":
        fs, cam = scenedefs.sponza_lod(add_lights=add_texture)
    elif name == "atrium":
        fs, cam = scenedefs.atrium()
    else:
        raise SystemExit("unknown scene %s" % name)
    r = PathTracing(0)
    try:
        r.UpdateSceneData(fs)
        r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], 256, 144))
        r.initSampler(256, 144, 0)
        r.render(256, 144, 5, 3)
        n_m, n_l = int(fs.desc.n_materials), int(fs.desc.n_lights)
        res = dict(scene=name, materials=n_m, lights=n_l, textures=int(fs.desc.n_textures), triangles=int(fs.desc.n_triangles))
        res["update_materials_one_ms"] = median_ms(lambda: r.updateMaterial(fs, first=n_m - 1, n=1), repeats)
        res["update_materials_all_ms"] = median_ms(lambda: r.updateMaterial(fs), repeats)
        if n_l:
            res["update_lights_all_ms"] = median_ms(lambda: r.updateLight(fs), repeats)
        tex = extra.get("tex")
        if tex is None:
            # (a scene built without the bench's texture: one of its own of that size, else its first -- the size is recorded)
            sized = [i for i, t in enumerate(fs.arrays["textures"]) if t.shape[:2] == (TEX, TEX)]
            tex = sized[0] if sized else (0 if int(fs.desc.n_textures) else None)
        if tex is not None:
            t = fs.arrays["textures"][tex]
            res["texture_size"] = [int(t.shape[1]), int(t.shape[0])]
            res["update_texture_ms"] = median_ms(lambda: r.UpdateTexture(fs, tex), repeats)
        res["update_rendering_config_ms"] = median_ms(lambda: r.UpdateSceneRenderingConfig(fs), repeats)
        res["upload_scene_ms"] = median_ms(lambda: r.UpdateSceneData(fs), repeats)
        r.render(256, 144, 5, 3)                    # the context is usable after all of it
        return res
    finally:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="sponza_lod,atrium")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per scene (a child process each)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(one_scene(args.child, args.repeats)), flush=True)
        return 0
    out = dict(workload="scene edits vs re-upload, frames idle, wall ms per synchronous call",
               protocol="one warm-up call, median of %d" % args.repeats, scenes=[])
    rc = 0
    for s in args.scenes.split(","):
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", s, "--repeats", str(args.repeats)],
                               capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            out["scenes"].append(dict(scene=s, error="timed out after %d s" % args.timeout))
            rc = 1
            break                                   # a hang: nothing more is started on the GPU
        if p.returncode != 0:
            out["scenes"].append(dict(scene=s, error="exit status %d" % p.returncode, stderr=p.stderr[-400:]))
            rc = 1
            break
        out["scenes"].append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
