#!/usr/bin/env python
"""bench.py -- headline benchmark of the MI355X path-tracing integrator.

Metric (BASELINE.json): Mrays/sec + ms/frame on "Sponza 1080p 1spp 5-bounce" at 1/2/4/8 GPUs, where
"Mrays/sec" is the reference's own definition W*H*spp/1e6/seconds (primary samples per second,
src/device_renderer/main.cpp:250).  The full sponza.obj/.sbvh are missing blobs in the reference
snapshot, so the workload is the reference's sponza_lod.obj + reference-built sponza_lod.sbvh with
GGX materials, textures and a synthetic IBL (aten_amd/scene/scenedefs.py:sponza_lod).

A step = one frame (one pass of the radiance loop over every pixel).  The scene, seeds and path
state are resident in HBM before the timed region.  With N > 1 the screen is sharded in 8x8 tiles
(tile t -> rank t % N), every rank renders its tiles and the tile buffers are all-gathered over
RCCL and assembled into the full frame on every rank ("strong" scaling: the image is fixed).  The
exchange of frame f runs on a communication stream while the renderer's stream traces frame f + 1;
the timed region ends only when the last frame is assembled on every rank.

A plain run sets up, warms up, times the K steps once, writes the outputs of the timed path when
--dump-outputs is given, and prints the result line.  --full adds everything else the benchmark
measures or checks: the repeated timed regions (median), frame latency, per-kernel times, the
roofline, path regeneration beside the serial loop, the CPU baseline, the film hash and the
unsharded re-render with N > 1, and on the default workload the atrium companion and the two
other trees.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scene sponza|cornell] [--dump-outputs DIR] [--full [--no-cpu-baseline]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md); 6290 GB/s measured copy peak


def algorithmic_bytes(nodes, tris, rays):
    """48 B per node visit, 80 B per triangle test (32 B TriangleParameter + 3 x 16 B
    positions), plus the per-ray state round trip of the trace kernel (32 B ray in, 24 B hit out)."""
    return 48 * nodes + 80 * tris + 56 * rays


L2_PEAK_GBS = 34500.0      # aggregate L2 bandwidth, MI355X_MICROARCH.md (L2 section)
OUTPUT_BUDGET_BYTES = 60_000_000       # --dump-outputs: all files together stay below 64 MB


def write_outputs(d, arrays):
    """--dump-outputs: every array as d/<name>.npy in float32.  An [H, W, C] array larger than its share of the budget is stored
    as a fixed, seeded sample of its pixels (<name>.npy: [k, C], pixel order) with their flat indices in <name>_index.npy."""
    os.makedirs(d, exist_ok=True)
    share = OUTPUT_BUDGET_BYTES // max(len(arrays), 1)
    for name, a in arrays.items():
        a = np.ascontiguousarray(a, np.float32)
        if a.nbytes > share:
            px = a.reshape(a.shape[0] * a.shape[1], -1)
            k = share // (px.shape[1] * 4 + 8)
            idx = np.sort(np.random.default_rng(0).choice(len(px), k, replace=False))
            np.save(os.path.join(d, name + "_index.npy"), idx.astype(np.float64))
            a = px[idx]
        np.save(os.path.join(d, name + ".npy"), a)


def profile_counters(scene, w, h, spp, depth, svgf, brk_multi=False):
    """Per-launch PMC averages of this workload's kernels from the committed passes (profiles/*counters*.json, written by
    tools/pmc_to_json.py from `rocprofv3 --pmc` runs of this same command): bench.py cannot collect PMC counters itself
    (they need the profiler around the process), so the fractions below combine those counters with the launch
    durations measured live here.  None when no committed profile matches the workload."""
    import glob
    from aten_amd.build import kernel_sources_sha16, build_id, loaded_build_id
    # (brk_multi: several samples per pixel with the CPU renderer's break-on-terminate sample loop -- its own work, its own counters)
    tag = "%s %dx%d %dspp %d-bounce%s%s" % (scene, w, h, spp, depth, " svgf" if svgf else "", " break" if brk_multi else "")
    sha = kernel_sources_sha16()
    # the binary that is being timed (ATEN_AMD_LIB may point at a variant build): counters count only if they were taken on
    # THIS binary, and this binary is what the tree's sources build (hash + flags compiled into it: atn_build_id)
    loaded = loaded_build_id()
    best, stale = None, None
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*counters*.json"))):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("workload", "") != tag:
            continue
        # counters are only valid for the kernels they were taken on: the record carries the hash of aten_amd/csrc +
        # include/ at collection time; a file from other sources is REFUSED (named in the output, not used)
        if d.get("kernel_sources_sha16") == sha and d.get("build_id", build_id()) == loaded and loaded.split("|")[0] == sha:
            best = (os.path.relpath(f, ROOT), d)
        else:
            stale = os.path.relpath(f, ROOT)
    return best, stale, sha


def load_calibration():
    """Measured ceilings of the counters the roofline is built from (tools/valu_calib.hip -> profiles/*calibration.json)."""
    import glob
    import hashlib
    fs = sorted(glob.glob(os.path.join(ROOT, "profiles", "*calibration.json")))
    if not fs:
        return None, None
    cal = json.load(open(fs[-1]))
    # ceilings count only if they were measured with the micro-benchmarks that are in the tree (content hash of
    # tools/valu_calib.hip recorded by tools/calib_to_json.py; r03's record predates the field and is taken as it is)
    try:
        now = hashlib.sha256(open(os.path.join(ROOT, "tools", "valu_calib.hip"), "rb").read()).hexdigest()[:16]
    except OSError:
        now = None
    if cal.get("calib_source_sha16") and now and cal["calib_source_sha16"] != now:
        return os.path.relpath(fs[-1], ROOT), {"ceilings": {}, "refused": "measured with another tools/valu_calib.hip (%s, tree has %s)" % (cal["calib_source_sha16"], now)}
    return os.path.relpath(fs[-1], ROOT), cal


def kernel_entry(counters, prefix):
    if not counters or not counters[0]:
        return None
    counters = counters[0]
    # several instantiations may share the prefix (e.g. the first launch of a sample runs k_trace_fused<false, .>, the
    # other five k_trace_fused<true, .>): the one with the most launches is the kernel the roofline is about
    best = None
    for k, e in counters[1]["kernels"].items():
        if k.startswith(prefix) and (best is None or e.get("launches_sampled", 0) > best.get("launches_sampled", 0)):
            best = e
    return best


def usable_cpus():
    """Host threads this process can really run at once: the affinity mask capped by the cgroup CPU quota (the GPU
    boxes report 256 logical CPUs but run the container under `cpu.max = 1600000 100000`, i.e. 16 CPUs; an OpenMP
    team wider than the quota is throttled and gets SLOWER: 64 threads 2.1, 256 threads 0.8 Mrays/s on sponza_lod)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(-(-int(quota) // int(period)))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, -(-q // p)))
        except Exception:
            pass
    return n


def needs_self_launch(gpus, mgpu, env):
    """True when bench.py was started as a plain process but asked for several GPUs in the one-rank-per-GPU mode."""
    return gpus > 1 and not mgpu and "WORLD_SIZE" not in env


def launcher_cmd(gpus, argv, port=None):
    """The command the driver itself uses for N > 1: torch.distributed.run, one rank per GPU, rendezvous on 127.0.0.1."""
    if port is None:
        import socket
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus),
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def main_mgpu(args):
    """One process drives every GPU through atn_mgpu_* (no torch.distributed): the path a C++ aten application takes."""
    import torch
    from aten_amd.renderer import MultiGpuPathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera
    W, H, spp, depth, rr = args.width, args.height, args.spp, args.depth, 3
    fs, cam = {"sponza": scenedefs.sponza_lod, "atrium": scenedefs.atrium, "cornell": scenedefs.cornell_box}[args.scene]()
    n_shards = args.shards or args.gpus
    devices = [i % args.gpus for i in range(n_shards)]
    m = MultiGpuPathTracing(devices)
    m.UpdateSceneData(fs)
    m.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H))
    m.initSampler(W, H, 0)
    m.set_frames_in_flight(min(args.frames_in_flight, 2))      # the node renderer double-buffers its gather
    brk = not args.all_samples
    for i in range(args.warmup):
        m.render(W, H, depth, rr, spp=spp, frame=i, break_on_terminate=brk, download=False)
    m.reset()
    m.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        m.render(W, H, depth, rr, spp=spp, frame=i, break_on_terminate=brk, download=False)
    m.synchronize()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump or args.dump_outputs:
        film = m.download_film()
        if args.dump:
            np.save(args.dump, film)
        if args.dump_outputs:
            write_outputs(args.dump_outputs, {"film": film})
    print(json.dumps({
        "metric": "Mrays/sec (W*H*spp/1e6/s, reference definition)", "value": round(W * H * spp / 1e6 / (elapsed / args.steps), 3),
        "unit": "Mrays/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "%s %dx%d %dspp %d-bounce" % (args.scene, W, H, spp, depth), "shards": n_shards, "devices": m.shard_devices(),
                   "sharding": "8x8 screen tiles, tile %% %d, one process, atn_mgpu_render: peer-copy gather into GPU 0" % n_shards}}))
    m.close()



def run_workload(args, cfg, ctx):
    """One benchmark workload end to end: W warm-up frames and the timed K frames; with cfg["full"] also the repeated timed
    regions, path regeneration beside them, the same frames with ONE frame in flight (latency), the same frames with HIP events,
    a counting pass, an isolated-kernel pass, the CPU baseline.  Returns the result dict on rank 0 (None elsewhere).  cfg:
    scene, width, height, spp, depth, svgf, all_samples, frames_in_flight, experiment, cpu_baseline, full, dump, dump_outputs;
    ctx: torch, dist, rank, local_rank, world, use_dist."""
    torch, dist = ctx["torch"], ctx["dist"]
    rank, local_rank, world, use_dist = ctx["rank"], ctx["local_rank"], ctx["world"], ctx["use_dist"]
    from aten_amd.interop import tensor_from_ptr
    from aten_amd.renderer import PathTracing
    from aten_amd.scene import scenedefs
    from aten_amd.scene.camera import create_camera

    scene = cfg["scene"]
    W, H, spp, depth, rr = cfg["width"], cfg["height"], cfg["spp"], cfg["depth"], 3
    svgf, steps, warmup = cfg["svgf"], args.steps, args.warmup
    in_flight = cfg["frames_in_flight"]
    if scene == "sponza":
        ex = set(x for x in cfg.get("experiment", "").split(",") if x)
        fs, cam = scenedefs.sponza_lod(textures="notex" not in ex, ibl="noibl" not in ex)
        workload = "sponza_lod %dx%d %dspp %d-bounce GGX+IBL, reference-built sponza_lod.sbvh (stand-in for missing sponza.obj)" % (W, H, spp, depth)
        if ex:
            workload += " EXPERIMENT " + "+".join(sorted(ex))
    elif scene == "sponza_own_tree":
        fs, cam = scenedefs.sponza_lod(use_sbvh=False)
        workload = "sponza_lod %dx%d %dspp %d-bounce GGX+IBL, tree built by atns_build_blas (split BVH)" % (W, H, spp, depth)
    elif scene == "sponza_ref_tree_opt":
        fs, cam = scenedefs.sponza_lod(use_sbvh=True, optimize_sbvh=True)
        workload = "sponza_lod %dx%d %dspp %d-bounce GGX+IBL, reference-built sponza_lod.sbvh through atns_optimize_nodes" % (W, H, spp, depth)
    elif scene == "atrium":
        fs, cam = scenedefs.atrium()
        workload = ("procedural atrium (%d triangles, Disney + Sponza textures + IBL + area light; synthetic Sponza-class scale-up, stand-in "
                    "for the missing Crytek Sponza blob) %dx%d %dspp %d-bounce%s" % (len(fs.arrays["triangles"]), W, H, spp, depth,
                                                                                 " all samples traced" if cfg["all_samples"] else ""))
    else:
        fs, cam = scenedefs.cornell_box()
        workload = "cornell box %dx%d %dspp %d-bounce NEE" % (W, H, spp, depth)
    brk = not cfg["all_samples"]
    camera = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)

    dev = "cuda:%d" % local_rank
    r = PathTracing(local_rank)
    r.UpdateSceneData(fs)
    n_planar = r.planar_area_lights()
    n_twins = r.anyhit_twins()      # bottom-level lists whose any-hit rays walk a second threading of the same tree (films do not depend on it)
    r.updateCamera(camera)
    r.initSampler(W, H, 0)
    r.setScreenShard(rank, world)
    if svgf:
        in_flight = min(in_flight, 2)   # SVGF hands a frame over through two slots: 2 in flight is its depth
    if use_dist:
        in_flight = min(in_flight, 3)   # the exchange stream wants a hardware queue of its own: 3 banks + 1 = the 4 there are
    r.set_frames_in_flight(in_flight)

    # Exchange step with N > 1: every rank contributes its tile buffer (RCCL all_gather over xGMI) and assembles the
    # full frame.  The exchange of frame f runs on its own stream while the renderer's stream already traces frame
    # f + 1 (two staging / gather buffers, events both ways); no host synchronisation inside a step.
    ext_streams = {}        # the renderer's stream of the frame just enqueued (one per bank of frames in flight)
    # HIP streams share a handful of hardware queues (4 under RCCL) and two streams on one queue run one after the other.
    # The renderer measures which of its bank streams run side by side (atn_set_frames_in_flight) and hands out a stream
    # for the exchange that has, if one is left, a queue of its own (atn_side_stream): a torch pool stream lands on SOME
    # queue, possibly a bank's, and the all_gather -- a cross-rank synchronisation point -- would then wait behind that bank's
    # trace kernels and hold its queue meanwhile.  (Synchronous c10d collectives are launched on the current stream.)
    comm_stream = torch.cuda.ExternalStream(r.side_stream_ptr(), device=dev) if use_dist else None
    stage, gathered, ev_ready, ev_free = [None, None], [None, None], [None, None], [None, None]
    full = [None]

    if cfg.get("shade_math") == "relaxed":
        r.set_shade_math(True)      # --shade-math relaxed: NOT the parity path (atn_set_shade_math), named in config.shade_math
    regen_timed = int(cfg.get("regen_timed") or 0)      # --regen K: the timed steps ARE regenerated bursts of K frames
    if regen_timed:
        r.set_regeneration(True)

    def step(frame, profile):
        if svgf:
            r.svgf_render(W, H, depth, rr, spp=spp, frame=frame, compute_motion=True, download=False, profile=profile)
            return
        if regen_timed:
            # (a step is still one frame: every K-th step enqueues the burst that holds it)
            if frame % regen_timed == 0:
                r.render_burst(W, H, regen_timed, depth, rr, spp=spp, frame=frame, progressive=True, break_on_terminate=brk, download=False, profile=profile)
            return
        r.render(W, H, depth, rr, spp=spp, frame=frame, progressive=True, break_on_terminate=brk, download=False,
                 profile=profile)
        if use_dist:
            n = r.tile_slots()
            k = frame & 1
            if stage[k] is None:
                stage[k] = torch.empty((n, 4), dtype=torch.float32, device=dev)
                gathered[k] = torch.empty((world * n, 4), dtype=torch.float32, device=dev)
                ev_ready[k] = torch.cuda.Event()
                ev_free[k] = torch.cuda.Event()
                ev_free[k].record(comm_stream)
            if full[0] is None:
                full[0] = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
            sp = r.stream_ptr()
            if sp not in ext_streams:
                ext_streams[sp] = torch.cuda.ExternalStream(sp, device=dev)
            ext_stream = ext_streams[sp]
            with torch.cuda.stream(ext_stream):
                ext_stream.wait_event(ev_free[k])           # the exchange of frame f - 2 has read stage[k]
                stage[k].copy_(tensor_from_ptr(r.tile_device_ptr(), (n, 4), dev))
                ev_ready[k].record(ext_stream)
            with torch.cuda.stream(comm_stream):
                comm_stream.wait_event(ev_ready[k])
                dist.all_gather_into_tensor(gathered[k], stage[k])
                r.assemble_tiles(gathered[k].data_ptr(), world, full[0].data_ptr(), comm_stream.cuda_stream)
                ev_free[k].record(comm_stream)

    def sync_all():
        r.synchronize()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    host_enqueue = [0.0]

    def timed(n):
        sync_all()
        t0 = time.perf_counter()
        for i in range(n):
            step(i, False)      # the timed region carries no instrumentation: no event records, no counters
        host_enqueue[0] = time.perf_counter() - t0      # the host's share: when it returns from the last enqueue
        sync_all()
        e = time.perf_counter() - t0
        if use_dist:
            t = torch.tensor([e], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            e = float(t.item())
        return e

    for i in range(warmup):
        step(i, False)
    # The timed region is EXACTLY K steps between barriers + synchronisations.  A plain run times it once; with --full it is
    # timed `repeats` times over (each from a reset film) and `value` is the MEDIAN: one 20-step region is 84 ms, noise
    # +-1-2 %, the same size as a round's gain
    repeats = max(1, args.repeats)
    region_s = []
    for _ in range(repeats):
        r.reset()
        region_s.append(timed(steps))
    # --repeats 0 ... no: a SHORT region (the driver's 20 steps are 70 ms) is repeated until the timed regions add up to
    # `--min-timed-seconds` of GPU work (--full: default 2 s, at most 64 repeats): a steadier median, and a GPU that an outside
    # sampler can see busy.  Every rank takes the same decision (the first region's duration is the max over ranks).
    if args.min_timed_seconds > 0 and region_s[0] > 0:
        want = int(min(64, np.ceil(args.min_timed_seconds / max(region_s[0], 1e-6))))
        if use_dist:
            tw = torch.tensor([want], dtype=torch.int64, device=dev)
            dist.broadcast(tw, 0)
            want = int(tw.item())
        while len(region_s) < want:
            r.reset()
            region_s.append(timed(steps))
        repeats = len(region_s)
    elapsed = float(np.median(region_s))
    host_enqueue_ms = 1e3 * host_enqueue[0] / steps
    ms_per_step = 1e3 * elapsed / steps
    mrays = W * H * spp / 1e6 / (elapsed / steps)
    # what the timed path computed in its last step, as its caller receives it: the film (K progressive frames from a reset film;
    # with N > 1 the frame assembled on rank 0) or, with SVGF, the filtered frame
    is_full = cfg.get("full", False)
    final_img = None
    if rank == 0 and not svgf and (is_full or cfg.get("dump") or cfg.get("dump_outputs")):
        final_img = full[0].cpu().numpy() if use_dist else r.download_film()
    if rank == 0 and cfg.get("dump_outputs"):
        write_outputs(cfg["dump_outputs"], {"svgf_output": r.svgf_buffer("output")} if svgf else {"film": final_img})
    # the film's hash goes into the line, so that the N = 1, 2, 4, 8 records of a scaling run can be held against each other
    # (the image does not depend on the sharding)
    import hashlib
    film_sha256 = None
    if is_full and final_img is not None:
        film_sha256 = hashlib.sha256(np.ascontiguousarray(final_img).tobytes()).hexdigest()
    if final_img is not None and cfg.get("dump"):
        np.save(cfg["dump"], final_img)
    final_img = None

    # what the collective layer saw: backend, world, and the device every rank drove (PCI bus id: distinct GPUs, not one GPU
    # N times) -- gathered while all ranks are still in step
    def gather_dist_info():
        if not use_dist:
            return None
        p = torch.cuda.get_device_properties(local_rank)
        mine = {"rank": rank, "local_rank": local_rank, "device_index": torch.cuda.current_device(), "name": p.name,
                "pci_bus_id": ("%04x:%02x:%02x" % (getattr(p, "pci_domain_id", 0), p.pci_bus_id, getattr(p, "pci_device_id", 0))) if hasattr(p, "pci_bus_id") else None,
                "uuid": str(getattr(p, "uuid", "")) or None, "tile_slots": int(r.tile_slots())}
        devices = [None] * world
        dist.all_gather_object(devices, mine)
        info = {"backend": dist.get_backend(), "world": dist.get_world_size(), "devices": devices,
                "distinct_devices": len(set((d["pci_bus_id"], d["uuid"]) for d in devices))}
        if info["backend"] == "nccl" and info["distinct_devices"] != world:
            # one rank per GPU is the contract: RCCL ranks sharing a device would make every number below meaningless
            raise SystemExit("bench.py: %d ranks drive %d distinct GPUs (%s)" % (world, info["distinct_devices"], devices))
        return info

    metric = ("Mrays/sec (W*H*spp/1e6/s, reference definition), Sponza 1080p 1spp 5-bounce" if (scene == "sponza" and (W, H, spp, depth) == (1920, 1080, 1, 5) and not svgf)
              else "Mrays/sec (W*H*spp/1e6/s, reference definition)")
    config = {"workload": workload, "width": W, "height": H, "spp": spp, "max_depth": depth, "rr_depth": rr,
              "sharding": "8x8 screen tiles, tile %% %d, RCCL all_gather of tile buffers" % world if world > 1 else "none",
              "frames_in_flight": in_flight, "shade_math": cfg.get("shade_math", "strict"),
              "regeneration": {"enabled_in_timed_region": True, "burst_frames": regen_timed} if regen_timed else None,
              "triangles": int(len(fs.arrays["triangles"])), "bvh_nodes": int(sum(len(n) for n in fs.arrays["bvh_lists"])),
              "anyhit_twins": n_twins, "planar_area_lights": n_planar}
    if not is_full:
        # a plain run: the headline figure of the K timed steps and nothing else (--full measures and checks the rest)
        dist_info = gather_dist_info()
        out = None
        if rank == 0:
            out = {"metric": metric, "value": round(mrays, 3), "unit": "Mrays/s", "n_gpus": world, "steps": steps, "warmup": warmup,
                   "ms_per_step": round(ms_per_step, 4), "repeats": repeats, "ms_per_step_repeats": [round(1e3 * t / steps, 4) for t in region_s],
                   "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                   "dist": dist_info, "config": config}
        r.close()
        return out

    # Path regeneration (atn_set_regeneration / atn_render_burst) beside the serial loop: the same K frames from
    # a reset film as bursts of `regen_burst` frames in one pool of path slots, same frames in flight.  OFF in the timed region above
    # unless --regen is given: measured, it does not win on these workloads -- the line carries both numbers and the film check.
    regen_info = None
    regen_burst = int(cfg.get("regen_burst", 8))
    if not svgf and not use_dist and regen_burst > 0 and not cfg.get("regen_timed"):
        nb = max(1, steps // regen_burst)

        def regen_region():
            r.reset()
            sync_all()
            t0 = time.perf_counter()
            for b in range(nb):
                r.render_burst(W, H, regen_burst, depth, rr, spp=spp, frame=b * regen_burst, progressive=True, break_on_terminate=brk, download=False)
            sync_all()
            return time.perf_counter() - t0
        r.set_regeneration(True)
        regen_region()
        ts = [regen_region() for _ in range(3)]
        regen_film = hashlib.sha256(np.ascontiguousarray(r.download_film()).tobytes()).hexdigest() if nb * regen_burst == steps else None
        q, sh = r.regen_stage_counts()
        r.set_regeneration(False)
        regen_ms = 1e3 * float(np.median(ts)) / (nb * regen_burst)
        regen_info = {"enabled_in_timed_region": False, "burst_frames": regen_burst, "ms_per_frame": round(regen_ms, 4),
                      "serial_ms_per_frame": round(1e3 * elapsed / steps, 4), "speedup": round(1e3 * elapsed / steps / regen_ms, 4),
                      "film_equals_serial": (regen_film == film_sha256) if regen_film else None,
                      "stages": int(len(q)), "mean_closest_rays_per_stage": round(float(q[q > 0].mean()) if (q > 0).any() else 0.0),
                      "path_slots": int(r.tile_slots())}

    # the same K frames with ONE frame in flight: what a caller that waits for every frame sees (frame LATENCY); `value`
    # above is THROUGHPUT with `in_flight` frames overlapping (progressive accumulation never waits for a frame)
    latency_ms = None
    if in_flight > 1:
        r.set_frames_in_flight(1)
        r.reset()
        for i in range(min(warmup, 2)):
            step(i, False)
        r.reset()
        latency_ms = 1e3 * float(np.median([timed(steps) for _ in range(min(repeats, 3))])) / steps
        r.set_frames_in_flight(in_flight)

    # the same K frames once more with every launch bracketed by HIP events on the stream it runs on: per-kernel
    # durations of the timed workload, measured live (the events cost ~2 % of a frame, which is why `value` is not
    # taken from this region)
    r.reset()
    r.reset_kernel_times()
    sync_all()
    t1 = time.perf_counter()
    for i in range(steps):
        step(i, True)
    sync_all()
    elapsed_events = time.perf_counter() - t1
    ktimes = r.kernel_times()

    # work counters of the same frames (untimed pass) for the roofline model
    r.reset()
    tot = dict(closest_rays=0, shadow_rays=0, hits=0, closest_nodes=0, closest_tris=0, shadow_nodes=0, shadow_tris=0)
    n_count = min(steps, 4)
    for i in range(n_count):
        r.render(W, H, depth, rr, spp=spp, frame=i, progressive=True, break_on_terminate=brk, download=False,
                 count_stats=True)
        st = r.stats()
        for k in tot:
            tot[k] += st[k]
    per_frame = {k: v / n_count for k, v in tot.items()}

    # the same frames once more with one kernel in flight at a time: per-kernel durations of isolated kernels
    # (in the timed region up to three batches of the frame overlap on separate streams, so a launch shares the GPU)
    r.set_path_batches(1)
    r.set_frames_in_flight(1)
    r.reset()
    r.reset_kernel_times()
    n_excl = min(steps, 10)
    for i in range(n_excl):
        if svgf:
            r.svgf_render(W, H, depth, rr, spp=spp, frame=i, compute_motion=True, download=False, profile=True)
        else:
            r.render(W, H, depth, rr, spp=spp, frame=i, progressive=True, break_on_terminate=brk, download=False, profile=True)
    r.synchronize()
    ktimes_excl = r.kernel_times()
    r.set_path_batches(3)
    r.set_frames_in_flight(in_flight)      # (SVGF: the path pass of frame f + 1 overlaps the filters of frame f)

    frames_prof = steps
    kernel_count_batches = max(1, round(ktimes["gen_path"][1] / max(frames_prof * spp, 1)))
    if ktimes["trace_fused"][1]:
        # the frame's trace work runs as depth + 1 launches of k_trace_fused (shadow rays of bounce b + closest-hit
        # rays of bounce b + 1): that kernel is the dominant one
        dominant, tkey = "k_trace_fused", "trace_fused"
        nodes = per_frame["closest_nodes"] + per_frame["shadow_nodes"]
        tris = per_frame["closest_tris"] + per_frame["shadow_tris"]
        rays = per_frame["closest_rays"] + per_frame["shadow_rays"]
    else:
        dominant, tkey = "k_trace_closest", "trace_closest"
        nodes, tris, rays = per_frame["closest_nodes"], per_frame["closest_tris"], per_frame["closest_rays"]
    bytes_per_frame = algorithmic_bytes(nodes, tris, rays)
    own_bytes_per_frame = 32 * (nodes - tris) + 48 * tris + 56 * rays       # this layout: 32-B inner records, 48-B leaf records
    tc_ms, tc_n = ktimes[tkey]
    launches_per_frame = max(tc_n / max(frames_prof, 1), 1)
    avg_launch_ms = tc_ms / max(tc_n, 1)
    # With frames in flight (or several batches per frame) a launch shares the GPU with other launches, so its wall
    # duration says nothing about how hard IT drives the machine; the roofline fractions use the duration of the same
    # launch with one kernel in flight at a time (the isolated pass above -- also the mode the PMC passes run in, the
    # profiler serialises dispatches), the overlapped duration is reported next to it.
    overlapped = kernel_count_batches > 1 or in_flight > 1
    iso_ms = (ktimes_excl[tkey][0] / ktimes_excl[tkey][1]) if ktimes_excl[tkey][1] else avg_launch_ms
    roof_ms = iso_ms if overlapped else avg_launch_ms
    avg_launch_s = max(roof_ms * 1e-3, 1e-12)
    scene_tag = {"sponza": "sponza_lod", "sponza_own_tree": "sponza_lod own tree", "sponza_ref_tree_opt": "sponza_lod reference tree optimised",
                 "cornell": "cornell", "atrium": "atrium"}[scene]
    prof, stale, sha = profile_counters(scene_tag, W, H, spp, depth, svgf, brk_multi=(spp > 1 and brk))
    pk = kernel_entry((prof,), dominant) if prof else None
    # The committed PMC record is of the UNSHARDED launch.  A rank of a world of N traces the rays of every N-th 8x8 tile: its
    # launch does 1/N of the record's accesses and bytes (interleaved tiles: equal shares within a per cent), in a duration that
    # is measured live on this rank.
    shard_scale = 1.0 / world
    if pk and world > 1:
        pk = dict(pk)
        for k in ("hbm_bytes", "hbm_read_bytes", "hbm_write_bytes", "hbm_bytes_lower", "l2_bytes_max"):
            if pk.get(k) is not None:
                pk[k] = pk[k] * shard_scale
    cal_file, cal = load_calibration()
    ceil = cal["ceilings"] if cal else {}
    # Candidate roofs for the dominant kernel, each a fraction <= 1 of a limit: HBM and L2 against the guide's peaks; the
    # per-CU L1 (TCP) and VALU issue against ceilings MEASURED on this chip with tools/valu_calib.hip (rocprofiler's derived
    # VALUBusy falls back to a gfx94x formula and reads up to 1.4 here: SQ_ACTIVE_INST_VALU is just 4 per instruction).
    # Counters: committed PMC passes of this workload (per launch) -- only if taken on THESE kernel sources; duration:
    # HIP events above.  `bound` names the largest fraction.
    fractions, extra = {}, {}
    if pk:
        scale = 1.0
        if pk.get("cycles") and roof_ms > 0:
            scale = shard_scale * (pk["cycles"] / 2.4e6) / roof_ms        # rates are per cycle of the PROFILED run: rescale by the duration ratio (and this rank's share)
        if "hbm_bytes" in pk:
            fractions["hbm"] = pk["hbm_bytes"] / avg_launch_s / 1e9 / HBM_PEAK_GBS
        if "l2_bytes_max" in pk:
            fractions["l2"] = pk["l2_bytes_max"] / avg_launch_s / 1e9 / L2_PEAK_GBS
        if pk.get("tcp_lane_accesses_per_cu_cycle") is not None and ceil.get("tcp_accesses_per_cu_cycle_rows"):
            # a 16-byte wave load occupies 64 lane slots of the TCP whatever its exec mask; the unit moves 4 slots (64 B) per clock
            slots = pk["tcp_lane_accesses_per_cu_cycle"] * scale / ceil["tcp_accesses_per_cu_cycle_rows"]
            tags = (pk.get("tcp_cache_accesses_per_cu_cycle") or 0.0) * scale / (ceil.get("tcp_cache_accesses_per_cu_cycle_random") or 1e30)
            fractions["l1"] = max(slots, tags)
            extra["l1_lane_slots"] = round(slots, 4); extra["l1_tag_lookups"] = round(tags, 4)
            extra["tcp_active"] = pk.get("tcp_active")
        if pk.get("valu_insts_per_simd_cycle") is not None and ceil.get("valu_insts_per_simd_cycle_fma"):
            fractions["valu"] = pk["valu_insts_per_simd_cycle"] * scale / ceil["valu_insts_per_simd_cycle_fma"]
            if ceil.get("valu_insts_per_simd_cycle_walkmix"):
                extra["valu_vs_packed_mix_ceiling"] = round(pk["valu_insts_per_simd_cycle"] * scale / ceil["valu_insts_per_simd_cycle_walkmix"], 4)
    bound = max(fractions, key=fractions.get) if fractions else "hbm"
    units = {"hbm": ("GB/s", HBM_PEAK_GBS), "l2": ("GB/s", L2_PEAK_GBS),
             "l1": ("TCP lane slots per CU per clock (16 B each)", ceil.get("tcp_accesses_per_cu_cycle_rows", 4.0)),
             "valu": ("VALU wave-instructions per SIMD per clock", ceil.get("valu_insts_per_simd_cycle_fma", 0.5))}
    frac = fractions.get(bound)
    roofline = {
        "kernel": dominant, "bound": bound,
        "achieved": round(frac * units[bound][1], 4) if frac is not None else None, "peak": units[bound][1], "unit": units[bound][0],
        "frac": round(frac, 4) if frac is not None else None,
        "traffic": round(pk["hbm_bytes"]) if pk and pk.get("hbm_bytes") is not None else None,
        "counters_scaled_by": shard_scale if world > 1 else None,
        "fractions": {k: round(v, 4) for k, v in fractions.items()},
        "fraction_detail": extra,
        "calibration": ({"file": cal_file, "git_head": cal.get("git_head"), "calib_source_sha16": cal.get("calib_source_sha16"), "refused": cal.get("refused"),
                         "ceilings_used": {k: ceil.get(k) for k in ("valu_insts_per_simd_cycle_fma", "valu_insts_per_simd_cycle_walkmix",
                                                                    "tcp_accesses_per_cu_cycle_rows", "tcp_cache_accesses_per_cu_cycle_random")}} if cal else None),
        "avg_launch_ms": round(avg_launch_ms, 5), "launches": tc_n,
        "roofline_launch_ms": round(roof_ms, 5),
        "algorithmic": {"bytes_per_launch": round(bytes_per_frame / launches_per_frame),
                        "GBps": round(bytes_per_frame / launches_per_frame / avg_launch_s / 1e9, 1),
                        "bytes_per_launch_this_layout": round(own_bytes_per_frame / launches_per_frame),
                        "GBps_this_layout": round(own_bytes_per_frame / launches_per_frame / avg_launch_s / 1e9, 1),
                        "note": "SURVEY 8(d): 48 B per node visit + 80 B per triangle test + 56 B per ray (reference layout); "
                                "this layout reads 32 B per inner visit and 48 B per leaf visit.  A rate, not a fraction of a roof: "
                                "the records are served by L1/L2"},
        "pmc": ({"file": prof[0], "kernel_sources_sha16": sha, "lane_utilisation": pk.get("lane_utilisation"), "l1_hit_rate": pk.get("l1_hit_rate"),
                 "l2_hit_rate": pk.get("l2_hit_rate"), "l1_stall": pk.get("l1_stall"),
                 "valu_insts_per_simd_cycle": pk.get("valu_insts_per_simd_cycle"),
                 "valu_useful": round(fractions["valu"] * pk["lane_utilisation"], 4) if pk.get("lane_utilisation") and "valu" in fractions else None,
                 "avg_launch_ms_profiled": round(pk["cycles"] / 2.4e6, 5) if pk.get("cycles") else None} if pk else
                {"file": None, "kernel_sources_sha16": sha, "loaded_build_id": __import__("aten_amd.build", fromlist=["x"]).loaded_build_id(), "refused_stale_file": stale,
                 "note": "no PMC record taken on these kernel sources (run tools/profile_round.sh): counter-derived fractions omitted"}),
        "note": "fractions: hbm = (FETCH_SIZE*2 + WRITE_SIZE) / t / 8 TB/s; l2 = TCC_REQ*128 B / t / 34.5 TB/s (upper bound); "
                "l1 = max(TCP_TOTAL_ACCESSES, i.e. 64 lane slots per 16-B wave load, / measured 3.95 slots per CU-clock; "
                "TCP_TOTAL_CACHE_ACCESSES / measured 1.62 tag lookups per CU-clock); valu = SQ_INSTS_VALU per SIMD-clock / measured "
                "0.35 (v_fma_f32, 8 waves per SIMD); DESIGN.md section 6",
    }
    # k_shade: the one kernel with material HBM traffic.  Compulsory bytes = the path state it must read and write once
    # per queue entry (80 B in: queue entry, ray, hit, throughput, seed; 16 B throughput out; per hit the next ray 32 B,
    # the shadow ray 48 B and two queue entries 8 B; per miss the contribution read-modify-write 32 B).
    sh_ms, sh_n = ktimes["shade"]
    sk = kernel_entry((prof,), "k_shade") if prof else None
    shade = None
    if sh_n:
        if overlapped and ktimes_excl["shade"][1]:
            sh_ms, sh_n = ktimes_excl["shade"][0] * (frames_prof / max(n_excl, 1)), ktimes_excl["shade"][1] * (frames_prof / max(n_excl, 1))
        sh_launch_s = sh_ms * 1e-3 / sh_n
        entries, hits = per_frame["closest_rays"], per_frame["hits"]
        comp = (96 * entries + 88 * hits + 32 * (entries - hits)) / max(sh_n / max(frames_prof, 1), 1)
        shade = {"kernel": "k_shade", "bound": "hbm", "avg_launch_ms": round(sh_launch_s * 1e3, 5), "launches": sh_n,
                 "compulsory_bytes_per_launch": round(comp),
                 "compulsory_GBps": round(comp / sh_launch_s / 1e9, 1),
                 "traffic": sk.get("hbm_bytes") if sk else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "achieved": round(sk["hbm_bytes"] / sh_launch_s / 1e9, 1) if sk and "hbm_bytes" in sk else None,
                 "frac": round(sk["hbm_bytes"] / sh_launch_s / 1e9 / HBM_PEAK_GBS, 4) if sk and "hbm_bytes" in sk else None,
                 "traffic_over_compulsory": round(sk["hbm_bytes"] / comp, 2) if sk and "hbm_bytes" in sk and comp else None,
                 "traffic_lower_bound": sk.get("hbm_bytes_lower") if sk else None,
                 "traffic_over_compulsory_lower_bound": round(sk["hbm_bytes_lower"] / comp, 2) if sk and sk.get("hbm_bytes_lower") and comp else None,
                 "traffic_note": "traffic = FETCH_SIZE x 2 + WRITE_SIZE (the guide's correction: streaming reads make 128-B requests tallied at 64 B); "
                                 "a random texel / environment-map lookup makes ONE 64-B request (measured: profiles/r03_calibration.json, "
                                 "k_cal_hbm_gather), so for this kernel the x2 over-counts the lookups: the truth lies between the two bounds"}
    roofline["shade"] = shade
    if overlapped:
        roofline["note"] += ("; %d frames in flight x %d batches per frame run on separate streams: avg_launch_ms (what rocprofv3 --kernel-trace "
                             "of this command shows) is the wall duration of a launch that shares the GPU, roofline_launch_ms the same launch "
                             "with one kernel in flight at a time, which the fractions use" % (in_flight, kernel_count_batches))
    kernel_ms_per_frame_isolated = {k: round(v[0] / max(n_excl, 1), 4) for k, v in ktimes_excl.items() if v[1]}
    # USEFUL work against what the chip can do at best for this access pattern: node visits (the oracle-checked counter) per CU per
    # microsecond over all trace launches of the frame (one kernel in flight), against the lane-hops per CU per microsecond a pure
    # pointer chase of two dependent 16-byte gathers per hop reaches through an L1-resident / L2-resident table (tools/valu_calib.hip:
    # k_cal_l1_chase, 5 waves per SIMD).  Unlike the unit fractions above this one goes UP when wasted instructions are removed.
    trace_iso_ms = sum(v for k, v in kernel_ms_per_frame_isolated.items() if k.startswith("trace_"))
    if trace_iso_ms > 0 and ceil.get("chase_l1_w5_lane_hops_per_cu_per_us"):
        visits = per_frame["closest_nodes"] + per_frame["shadow_nodes"]      # this rank's walks
        rate = visits / 256.0 / (trace_iso_ms * 1e3)
        roofline["useful"] = {"node_visits_per_cu_per_us": round(rate, 1),
                              "l1_resident_chase_ceiling": ceil["chase_l1_w5_lane_hops_per_cu_per_us"],
                              "l2_resident_chase_ceiling": ceil.get("chase_l2_w5_lane_hops_per_cu_per_us"),
                              "frac_of_l1_chase": round(rate / ceil["chase_l1_w5_lane_hops_per_cu_per_us"], 4),
                              "trace_ms_per_frame_isolated": round(trace_iso_ms, 4)}
    kernel_ms_per_frame = {k: round(v[0] / max(frames_prof, 1), 4) for k, v in ktimes.items() if v[1] or not k.startswith("svgf")}
    svgf_info = None
    if svgf:
        # compulsory HBM bytes per pixel and launch (every input plane read once, every output written once; the
        # filter taps themselves are L2 hits): a-trous reads normal+depth, albedo+id, colour+variance and writes one
        # plane (+ the temporary colour on the first and the output on the last iteration).  The launch duration is the
        # ISOLATED one (one kernel in flight): in the timed region the filters of frame f overlap the path pass of f + 1.
        px = W * H
        at_ms, at_n = ktimes_excl["svgf_atrous"]
        at_bytes = px * (48 + 16) + px * 32 / max(at_n / max(n_excl, 1), 1)
        at_launch_ms = at_ms / max(at_n, 1)
        ak = kernel_entry((prof,), "k_svgf_atrous") if prof else None
        svgf_info = {"passes_ms_per_frame": {k: kernel_ms_per_frame[k] for k in kernel_ms_per_frame if k.startswith("svgf")},
                     "passes_ms_per_frame_isolated": {k: v for k, v in kernel_ms_per_frame_isolated.items() if k.startswith("svgf")},
                     "atrous": {"bound": "hbm", "compulsory_bytes_per_launch": int(at_bytes), "avg_launch_ms_isolated": round(at_launch_ms, 5),
                                "achieved": round(at_bytes / (at_launch_ms * 1e-3) / 1e9, 1) if at_n else None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                "frac": round(at_bytes / (at_launch_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if at_n else None,
                                "traffic": ak.get("hbm_bytes") if ak else None},
                     "filter_ms_per_frame": round(sum(v for k, v in kernel_ms_per_frame.items() if k.startswith("svgf")), 4),
                     "filter_ms_per_frame_isolated": round(sum(v for k, v in kernel_ms_per_frame_isolated.items() if k.startswith("svgf")), 4)}
    ray_segments = per_frame["closest_rays"] + per_frame["shadow_rays"]

    cpu_baseline = None
    if rank == 0 and cfg["cpu_baseline"]:     # at any world size: the other ranks wait at the next collective (10 - 25 s)
        from oracle import orc     # the cpu_baseline leg is the only place bench.py touches oracle/
        # bounded sample of the same workload: the benchmarked frame itself (same scene / camera / seeds / size) when a
        # CPU frame takes seconds (1080p 1 spp: ~1.2 s with 16 threads); 1/6 linear resolution for the 4K 8-spp config,
        # whose full frame would take minutes
        cw, ch = W, H
        if W * H * spp > 4 * 1920 * 1080:
            cw, ch = max(W // 6, 8), max(H // 6, 8)
        ccam = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], cw, ch)
        cseeds = orc.init_sampler(cw, ch, 0)

        cpu_svgf = orc.Svgf() if svgf else None

        def cpu_frame(f, nthreads=0):
            if cpu_svgf is not None:
                cpu_svgf.render(fs, ccam, cseeds, cw, ch, depth, rr, spp=spp, frame=f, compute_motion=True, nthreads=nthreads)
            elif brk or spp == 1:
                orc.render(fs, ccam, cseeds, cw, ch, depth, rr, spp=spp, frame=f, nthreads=nthreads)
            else:       # every sample traced: spp passes of one sample (same work as the GPU's all-samples mode)
                for i in range(spp):
                    orc.render(fs, ccam, cseeds, cw, ch, depth, rr, spp=1, frame=f * spp + i, nthreads=nthreads)

        def cpu_median(nthreads, min_frames, budget_s):
            cpu_frame(0, nthreads)      # warm-up
            ts = []
            t_all = time.perf_counter()
            while (len(ts) < min_frames or time.perf_counter() - t_all < budget_s / 3) and time.perf_counter() - t_all < budget_s:
                t1 = time.perf_counter()
                cpu_frame(len(ts), nthreads)
                ts.append(time.perf_counter() - t1)
            return float(np.median(ts)), len(ts)

        n_cpu = usable_cpus()
        budget = cfg.get("cpu_budget_s", 16.0)
        med, nfr = cpu_median(n_cpu, 5 if budget >= 16 else 3, budget)
        cpu_baseline = {"value": round(cw * ch * spp / 1e6 / med, 4), "unit": "Mrays/s", "cores": n_cpu, "logical_cpus": orc.lib().orc_num_procs(),
                        "measured_at_world": world,
                        "kind": "port", "sample": ("the benchmarked frame itself: " if (cw, ch) == (W, H) else "reduced frame: ") + "%dx%d frames of the same scene/camera/seeds, %d frames, median; OpenMP parallel-for over rows like pathtracing.cpp:296-305, one thread per CPU the container may use (cgroup quota)" % (cw, ch, nfr),
                        "ms_per_frame_sample": round(1e3 * med, 2)}
        if cfg.get("cpu_8_threads", True):
            med8, nfr8 = cpu_median(8, 2, 8.0)      # the reference app's own setting (host_renderer/main.cpp:18-23,271)
            cpu_baseline["value_8_threads"] = round(cw * ch * spp / 1e6 / med8, 4)
            cpu_baseline["frames_8_threads"] = nfr8

    dist_info = gather_dist_info()

    # --verify-film: rank 0 renders the same K frames UNSHARDED once more and compares the film with the one the N ranks
    # assembled (byte for byte; the other ranks go on to the closing barrier)
    film_equals_single = None
    if cfg.get("verify_film") and rank == 0 and film_sha256 is not None and not svgf:
        r.setScreenShard(0, 1)
        r.set_frames_in_flight(in_flight)
        r.reset()
        for i in range(steps):
            r.render(W, H, depth, rr, spp=spp, frame=i, progressive=True, break_on_terminate=brk, download=False)
        r.synchronize()
        film_equals_single = hashlib.sha256(np.ascontiguousarray(r.download_film()).tobytes()).hexdigest() == film_sha256

    out = None
    if rank == 0:
        out = {
            "metric": metric,
            "value": round(mrays, 3), "unit": "Mrays/s", "n_gpus": world, "steps": steps, "warmup": warmup,
            "ms_per_step": round(ms_per_step, 4),
            "repeats": repeats, "spread": round(max(region_s) / min(region_s), 4),
            "ms_per_step_repeats": [round(1e3 * t / steps, 4) for t in region_s],
            "timing_note": "the K-step region (barrier + synchronise on both sides, max over ranks) timed `repeats` times from a reset film; value = median",
            "film_sha256": film_sha256, "film_equals_single_gpu": film_equals_single, "dist": dist_info,
            "ms_per_frame_latency": round(latency_ms, 4) if latency_ms is not None else round(ms_per_step, 4),
            "throughput_note": ("value / ms_per_step are THROUGHPUT with %d frames in flight (progressive accumulation enqueues frames back to back; "
                                "one frame's launch tails overlap the next frame's bulk); ms_per_frame_latency is the same K frames with one frame "
                                "in flight, i.e. what a caller that waits for each frame sees" % in_flight) if in_flight > 1 else "one frame in flight: throughput = latency",
            "ms_per_step_with_events": round(1e3 * elapsed_events / steps, 4),
            "host_enqueue_ms_per_step": round(host_enqueue_ms, 4),
            "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": dict(config, regeneration=config["regeneration"] or regen_info),
            "ray_segments_per_frame": round(ray_segments), "Mray_segments_per_s": round(ray_segments / 1e6 / (elapsed / steps), 2),
            "work_per_frame": {k: round(v) for k, v in per_frame.items()},
            "kernel_ms_per_frame": kernel_ms_per_frame,
            "kernel_ms_per_frame_isolated": kernel_ms_per_frame_isolated,
            "roofline": roofline,
            "svgf": svgf_info,
            "cpu_baseline": cpu_baseline,
        }
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed frames (default 200: a timed region of ~0.8 s; 20 for the 4K 8-spp config)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scene", default="sponza", choices=["sponza", "sponza_own_tree", "sponza_ref_tree_opt", "cornell", "atrium"])
    ap.add_argument("--config", default=None, choices=["c2", "c3", "c4", "c5"],
                    help="BASELINE.json config shortcuts: c2 = Cornell 1080p 1spp 5-bounce, c3 = Sponza 1080p 1spp 5-bounce "
                         "(default), c4 = 4K 8spp 8-bounce Disney + textures on the procedural atrium stand-in, "
                         "c5 = c3 + SVGF temporal/variance/a-trous passes (1 GPU)")
    ap.add_argument("--svgf", action="store_true", help="a step = SVGFRenderer::OnRender (path pass with AOVs + filter passes)")
    ap.add_argument("--all-samples", action="store_true",
                    help="with spp > 1: trace every sample (the CPU reference stops a pixel's sample loop at the first "
                         "terminated path, pathtracing.cpp:350-352; default reproduces that)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything beside the headline figure: repeated timed regions (median), frame latency, "
                         "per-kernel times, roofline, path regeneration beside the serial loop, CPU baseline, film hash, the unsharded "
                         "re-render with N > 1, and on the default workload the companion and the two other trees; a plain run times "
                         "the K steps once and prints the headline line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the timed path computed in its last step as DIR/<name>.npy (float32): "
                         "film.npy, the accumulated film [H, W, 4] (svgf_output.npy with --svgf); an output over the 64 MB budget "
                         "is a fixed, seeded sample of its pixels, with their indices in <name>_index.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--cpu-budget", type=float, default=0.0, help="seconds of CPU-baseline sampling (default 16, + 8 for the 8-thread sample; below 12 the 8-thread sample is skipped)")
    ap.add_argument("--no-companion", action="store_true",
                    help="with --full the default run (Sponza stand-in, 1 GPU) also times the 250 K-triangle procedural atrium at the same 1080p 1 spp "
                         "5-bounce protocol and reports it under `companion` (SURVEY 8(d): the stand-in AND a synthetic scale-up); this skips it")
    ap.add_argument("--no-own-tree", action="store_true",
                    help="with --full the default run also times the headline frames through the tree of the repo's own BVH builder (`own_tree`); this skips it")
    ap.add_argument("--experiment", default="", help="traffic experiments on the sponza scene, not a benchmark configuration: "
                    "'notex' (no textures), 'noibl' (white background instead of the environment map), 'notex,noibl'")
    ap.add_argument("--dump", default=None, help="write the final frame (npy) here")
    ap.add_argument("--frames-in-flight", type=int, default=4,
                    help="consecutive frames enqueued on rotating banks of path state and streams (atn_set_frames_in_flight): "
                         "one frame's launch tails overlap the next frame's bulk; 1 = strictly one frame at a time")
    ap.add_argument("--shade-math", default="strict", choices=["strict", "relaxed"],
                    help="relaxed: k_shade under the reference GPU build's --use_fast_math rules (atn_set_shade_math 1) -- an opt-in that leaves the parity path; "
                         "the line says so in config.shade_math")
    ap.add_argument("--regen", type=int, default=0,
                    help="K > 0: the timed steps are path-regenerated bursts of K progressive frames (atn_render_burst; --steps a multiple of K, one GPU); "
                         "default 0: the serial loop is timed (and with --full an 8-frame regenerated burst is measured beside it, config.regeneration)")
    ap.add_argument("--mgpu", action="store_true",
                    help="one process, every GPU behind the C-ABI (atn_mgpu_*: worker thread per GPU, peer-copy gather into "
                         "GPU 0) instead of one process per GPU + RCCL all_gather")
    ap.add_argument("--shards", type=int, default=0, help="with --mgpu: shard count when it differs from --gpus (shards then share GPUs)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend of the one-rank-per-GPU mode; nccl (= RCCL) is what is measured, gloo lets "
                         "several ranks SHARE a GPU (RCCL refuses that), which is how the tests run a world of two on a 1-GPU box")
    ap.add_argument("--repeats", type=int, default=None,
                    help="the K-step timed region is measured (at least) this many times; value = the median (default 1, 5 with --full)")
    ap.add_argument("--min-timed-seconds", type=float, default=None,
                    help="repeat the K-step region until the regions add up to this much time (0 = exactly --repeats); at most 64 repeats "
                         "(default 0, 2 with --full)")
    ap.add_argument("--verify-film", action="store_true",
                    help="with --full: after the timed region rank 0 renders the same K frames unsharded and reports film_equals_single_gpu "
                         "(on by default with more than one rank)")
    ap.add_argument("--no-verify-film", action="store_true", help="skip that check with more than one rank")
    ap.add_argument("--force-gather", action="store_true",
                    help="run the RCCL tile gather even with one rank (exercises the N>1 step on a 1-GPU box)")
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 5 if args.full else 1
    if args.min_timed_seconds is None:
        args.min_timed_seconds = 2.0 if args.full else 0.0
    if args.config == "c2":
        args.scene = "cornell"
    elif args.config == "c4":
        args.scene, args.width, args.height, args.spp, args.depth, args.all_samples = "atrium", 3840, 2160, 8, 8, True
        if args.steps is None:
            args.steps = 20
    elif args.config == "c5":
        args.svgf = True
    if args.steps is None:
        args.steps = 200 if args.width * args.height * args.spp <= 4 * 1920 * 1080 else 20
    if args.regen and (args.steps % args.regen or args.svgf or args.gpus > 1):
        ap.error("--regen K needs --steps to be a multiple of K, one GPU, and not --svgf")

    if needs_self_launch(args.gpus, args.mgpu, os.environ):
        # `python bench.py --gpus N` on its own: become the launcher the contract describes (one rank per GPU)
        os.execv(sys.executable, launcher_cmd(args.gpus, sys.argv[1:]))

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.mgpu:
        return main_mgpu(args)
    if world != args.gpus:
        args.gpus = world
    dist = None
    use_dist = world > 1 or args.force_gather
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if args.dist_backend == "gloo":
            local_rank = local_rank % torch.cuda.device_count()     # ranks may share a GPU (tests)
            torch.cuda.set_device(local_rank)
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))


    ctx = {"torch": torch, "dist": dist, "rank": rank, "local_rank": local_rank, "world": world, "use_dist": use_dist}
    cfg = {"scene": args.scene, "width": args.width, "height": args.height, "spp": args.spp, "depth": args.depth, "svgf": args.svgf,
           "all_samples": args.all_samples, "frames_in_flight": args.frames_in_flight, "experiment": args.experiment,
           "cpu_baseline": not args.no_cpu_baseline, "dump": args.dump, "dump_outputs": args.dump_outputs, "full": args.full, "regen_timed": args.regen, "shade_math": args.shade_math,
           **({"cpu_budget_s": args.cpu_budget, "cpu_8_threads": args.cpu_budget >= 12} if args.cpu_budget > 0 else {}),
           "verify_film": args.full and (args.verify_film or (world > 1 and not args.no_verify_film))}
    out = run_workload(args, cfg, ctx)

    # "sponza_lod for oracle-checked runs AND a synthetic scale-up for perf -- say which one every time".  The
    # headline stand-in is a 1.5 MB tree that lives in L1/L2; the atrium (250 K triangles, 17 MB of records) does not fit
    # an XCD's L2 and has real L2 / HBM traffic.  Same protocol, own roofline and CPU baseline, under `companion`.
    default_line = (args.scene == "sponza" and (args.width, args.height, args.spp, args.depth) == (1920, 1080, 1, 5) and not args.svgf
                    and not args.experiment and world == 1 and not use_dist)
    if args.full and default_line and not args.no_companion:
        ccfg = dict(cfg, scene="atrium", dump=None, dump_outputs=None, cpu_budget_s=9.0, cpu_8_threads=False)
        comp = run_workload(args, ccfg, dict(ctx, use_dist=False))
        if rank == 0 and comp is not None:
            keep = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "ms_per_frame_latency", "config", "ray_segments_per_frame",
                    "Mray_segments_per_s", "work_per_frame", "kernel_ms_per_frame_isolated", "roofline", "cpu_baseline")
            out["companion"] = {k: comp[k] for k in keep}
            out["companion"]["why"] = ("the headline stand-in (sponza_lod, 12 852 triangles) is cache-resident; this synthetic Sponza-class "
                                       "scale-up is the workload whose tree does not fit an XCD's L2")
            # the same in short inside `config` (the driver's record keeps config / roofline / cpu_baseline, not extra keys)
            out["config"]["companion"] = {"workload": "atrium %d triangles %dx%d %dspp %d-bounce" % (comp["config"]["triangles"], args.width, args.height, args.spp, args.depth),
                                          "value": comp["value"], "unit": comp["unit"], "ms_per_step": comp["ms_per_step"],
                                          "ms_per_frame_latency": comp["ms_per_frame_latency"],
                                          "roofline_bound": comp["roofline"]["bound"], "roofline_frac": comp["roofline"]["frac"],
                                          "cpu_baseline_value": (comp["cpu_baseline"] or {}).get("value")}
    if args.full and default_line and not args.no_own_tree:
        # the same headline frames through (a) the tree of the repo's OWN builder (csrc/host/bvh_builder.cpp) instead of the
        # reference-built sponza_lod.sbvh -- what a caller who ingests the OBJ through atns_* gets -- and (b) the reference-built
        # tree after the builder's post passes (atns_optimize_nodes: same boxes and leaves, re-arranged and re-threaded)
        ref_visits = max(out["work_per_frame"]["closest_nodes"] + out["work_per_frame"]["shadow_nodes"], 1) if rank == 0 else 1
        for key, sc in (("own_tree", "sponza_own_tree"), ("reference_tree_optimized", "sponza_ref_tree_opt")):
            ocfg = dict(cfg, scene=sc, dump=None, dump_outputs=None, cpu_baseline=False)
            own = run_workload(args, ocfg, dict(ctx, use_dist=False))
            if rank == 0 and own is not None:
                out[key] = {k: own[k] for k in ("value", "unit", "ms_per_step", "ms_per_frame_latency", "work_per_frame", "kernel_ms_per_frame_isolated", "film_sha256")}
                out[key]["workload"] = own["config"]["workload"]
                out[key]["bvh_nodes"] = own["config"]["bvh_nodes"]
                out["config"][key] = {"value": own["value"], "ms_per_step": own["ms_per_step"],
                                      "node_visits_vs_reference_tree": round((own["work_per_frame"]["closest_nodes"] + own["work_per_frame"]["shadow_nodes"]) / ref_visits, 4)}
    if args.full and rank == 0 and out is not None:
        parts = ["%s: %.1f Mrays/s, %.3f ms/frame, roofline %s %s" % (out["config"]["workload"][:40], out["value"], out["ms_per_step"], out["roofline"]["bound"], out["roofline"]["frac"])]
        if "companion" in out:
            c = out["companion"]
            parts.append("companion atrium: %.1f Mrays/s, %.3f ms/frame, roofline %s %s" % (c["value"], c["ms_per_step"], c["roofline"]["bound"], c["roofline"]["frac"]))
        if "own_tree" in out:
            parts.append("own-tree sponza_lod: %.1f Mrays/s, %.3f ms/frame" % (out["own_tree"]["value"], out["own_tree"]["ms_per_step"]))
        if "reference_tree_optimized" in out:
            parts.append("reference tree through atns_optimize_nodes: %.1f Mrays/s, %.3f ms/frame" % (out["reference_tree_optimized"]["value"], out["reference_tree_optimized"]["ms_per_step"]))
        out["summary"] = "; ".join(parts)        # last key: survives a reader that keeps only the tail of the line
        print("[bench] " + out["summary"], file=sys.stderr, flush=True)

    if use_dist:
        # every rank drains its own buffers (RCCL's banner sits in the C library's) BEFORE rank 0 writes the JSON line
        sys.stdout.flush()
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # RCCL writes "Hostname : ... / Librccl path : ..." into the C library's stdout buffer, which would otherwise be
        # flushed at exit, after the JSON line: drain both buffers first
        sys.stdout.flush()
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)      # the one JSON line, after every library has had its say


if __name__ == "__main__":
    main()
