"""bench.py as the driver runs it, on one GPU: the plain line and its outputs, the JSON contract of --full, the companion
workload, and -- with --force-gather -- the N > 1 exchange step (RCCL all_gather_into_tensor of the tile buffers +
atn_assemble_tiles_on) with a world of one, so that the multi-GPU bench path runs every round even when no 8-GPU node is
available."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(extra, tmp_path, name):
    dump = str(tmp_path / (name + ".npy"))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29571", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--no-companion", "--no-own-tree", "--min-timed-seconds", "0", "--dump", dump] + extra,
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    return json.loads(lines[-1]), np.load(dump)      # the JSON line is the LAST line of stdout, whatever RCCL printed before


@pytest.mark.gpu
def test_plain_line_times_k_steps_and_dumps_what_they_computed(tmp_path):
    """A plain run (no --full) times exactly --steps steps once and prints the headline line only; --dump-outputs writes the film
    of the last timed step, the same film --full's --dump writes, and the same inputs give the same outputs from run to run."""
    env = dict(os.environ)
    lines, films = [], []
    for i in range(2):
        out = tmp_path / ("out%d" % i)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(out)], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        lines.append(json.loads([l for l in p.stdout.decode().splitlines() if l.strip()][-1]))
        assert sorted(os.listdir(out)) == ["film.npy"]
        films.append(np.load(out / "film.npy"))
    for d in lines:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["repeats"] == 1 and len(d["ms_per_step_repeats"]) == 1
        assert d["ms_per_step"] == d["ms_per_step_repeats"][0] > 0
        assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert abs(d["value"] - 1920 * 1080 / 1e6 / (d["ms_per_step"] * 1e-3)) < 1e-3 * d["value"]
        assert "Sponza 1080p 1spp 5-bounce" in d["metric"] and "sponza_lod" in d["config"]["workload"]
        for k in ("roofline", "cpu_baseline", "companion", "own_tree", "ms_per_frame_latency", "film_sha256", "summary"):
            assert k not in d, k
    assert films[0].dtype == np.float32 and films[0].shape == (1080, 1920, 4)
    assert (films[0][..., 3] == 3).all()
    assert films[0].tobytes() == films[1].tobytes()
    _, film_full = run_bench([], tmp_path, "full")
    assert film_full.tobytes() == films[0].tobytes()


@pytest.mark.gpu
def test_force_gather_film_equals_plain_film(tmp_path):
    plain, film_plain = run_bench([], tmp_path, "plain")
    gath, film_gath = run_bench(["--force-gather"], tmp_path, "gather")
    assert film_plain.shape == (1080, 1920, 4)
    assert film_gath.tobytes() == film_plain.tobytes()
    assert (film_plain[..., 3] == 3).all()
    import hashlib
    for d in (plain, gath):
        assert d["n_gpus"] == 1 and d["steps"] == 3 and d["unit"] == "Mrays/s" and d["value"] > 0
        assert d["roofline"]["kernel"] == "k_trace_fused" and d["ms_per_frame_latency"] >= 0.9 * d["ms_per_step"]
        # the K-step region is timed `repeats` times, value is the median; the film's hash travels in the line
        # (a 3-frame region is ~12 ms and one host hiccup in one of the five doubles it -- seen once in r04 -- so the bound is on
        #  the three middle repeats, which a single outlier cannot move: they agree within 1.5 x)
        assert d["repeats"] == 5 and len(d["ms_per_step_repeats"]) == 5 and d["spread"] >= 1.0
        mid = sorted(d["ms_per_step_repeats"])[1:4]
        assert mid[2] <= 1.5 * mid[0], d["ms_per_step_repeats"]
        assert abs(d["ms_per_step"] - float(np.median(d["ms_per_step_repeats"]))) < 1e-3
        assert d["film_sha256"] == hashlib.sha256(film_plain.tobytes()).hexdigest()
    assert plain["dist"] is None
    # with the exchange step on, the line says what the collective layer saw
    assert gath["dist"]["backend"] == "nccl" and gath["dist"]["world"] == 1 and len(gath["dist"]["devices"]) == 1
    assert gath["dist"]["devices"][0]["rank"] == 0 and gath["dist"]["devices"][0]["tile_slots"] > 0


@pytest.mark.gpu
def test_default_line_carries_roofline_companion_and_cpu_baseline():
    env = dict(os.environ)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "4", "--warmup", "1"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    d = json.loads([l for l in p.stdout.decode().splitlines() if l.strip()][-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "companion", "ms_per_frame_latency"):
        assert k in d, k
    assert "sponza_lod" in d["config"]["workload"] and "atrium" in d["companion"]["config"]["workload"]
    # a 4-step region is ~15 ms: it is repeated until the timed regions add up to ~2 s (at most 64 times)
    assert d["repeats"] == 64 and len(d["ms_per_step_repeats"]) == 64
    for w in (d, d["companion"]):
        rf = w["roofline"]
        assert rf["bound"] in ("hbm", "l2", "l1", "valu") and rf["avg_launch_ms"] > 0
        assert rf["calibration"] and rf["calibration"]["file"].startswith("profiles/")
        # counters are used only when taken on these kernel sources; otherwise the record says which file was refused
        assert rf["pmc"]["kernel_sources_sha16"]
        if rf["pmc"]["file"] is None:
            assert rf["frac"] is None and "refused_stale_file" in rf["pmc"]
        else:
            assert 0 < rf["frac"] <= 1.0 and set(rf["fractions"]) >= {"hbm", "l2", "l1", "valu"}
        cb = w["cpu_baseline"]
        assert cb["kind"] == "port" and cb["value"] > 0 and cb["cores"] >= 1
    # the companion and the own-tree run in short inside `config` (the part of the line the driver's record keeps), and as the
    # LAST key of the line
    cc = d["config"]["companion"]
    assert cc["value"] == d["companion"]["value"] and cc["ms_per_step"] == d["companion"]["ms_per_step"] and "roofline_frac" in cc
    ot = d["own_tree"]
    assert "atns_build_blas" in ot["workload"] and ot["value"] > 0
    assert 0.8 < d["config"]["own_tree"]["node_visits_vs_reference_tree"] < 1.0
    ro = d["reference_tree_optimized"]
    assert "atns_optimize_nodes" in ro["workload"] and ro["bvh_nodes"] == d["config"]["bvh_nodes"]
    assert 0.8 < d["config"]["reference_tree_optimized"]["node_visits_vs_reference_tree"] < 1.0
    assert list(d)[-1] == "summary" and "companion atrium" in d["summary"] and "own-tree" in d["summary"]
    assert "[bench] " + d["summary"] in p.stderr.decode()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 7])
def test_ranks_sharing_the_gpu_render_the_single_rank_film(tmp_path, world):
    """The N > 1 bench path with a world of two (and of seven: a tile count that does not divide) on the hardware there is: the launcher command the driver uses
    (torch.distributed.run, one process per rank, rendezvous on 127.0.0.1), each rank renders its tiles (tile t -> rank
    t % world) with frames in flight, exchanges them every frame and assembles the frame -- with the gloo backend, because RCCL
    refuses two ranks on one device.  Rank 0's assembled film equals the single-rank film byte for byte."""
    _, film_plain = run_bench([], tmp_path, "plain1")
    dump = str(tmp_path / "two.npy")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(29573 + world), os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(world), "--dist-backend", "gloo", "--steps", "3",
           "--warmup", "1", "--repeats", "2", "--min-timed-seconds", "0", "--dump", dump] + (["--no-cpu-baseline"] if world != 2 else [])
    # (no --verify-film: with more than one rank it is on by default; the world of two also carries the CPU baseline, which
    #  rank 0 measures while the others wait -- the plain `bench.py --gpus N` line of the driver must be complete)
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip().startswith("{")]
    d = json.loads(lines[-1])
    assert len(lines) == 1, "only rank 0 prints the JSON line"
    assert d["n_gpus"] == world and d["steps"] == 3 and d["scaling"] == "strong" and d["value"] > 0
    film_two = np.load(dump)
    assert film_two.tobytes() == film_plain.tobytes()
    # the line proves itself: backend, world and device of every rank as torch.distributed saw them, the film's hash, and rank
    # 0's own unsharded re-render of the same frames
    import hashlib
    di = d["dist"]
    assert di["backend"] == "gloo" and di["world"] == world and sorted(x["rank"] for x in di["devices"]) == list(range(world))
    assert di["distinct_devices"] == 1                       # the ranks of this test share the box's one GPU
    assert sum(x["tile_slots"] for x in di["devices"]) >= 1920 * 1080
    assert d["film_sha256"] == hashlib.sha256(film_plain.tobytes()).hexdigest()
    assert d["film_equals_single_gpu"] is True
    assert d["config"]["frames_in_flight"] >= 1
    if world == 2:
        cb = d["cpu_baseline"]
        assert cb["kind"] == "port" and cb["value"] > 0 and cb["measured_at_world"] == 2
    else:
        assert d["cpu_baseline"] is None
    assert d["repeats"] == 2 and d["spread"] >= 1.0
    rf = d["roofline"]
    assert rf["kernel"] == "k_trace_fused" and rf["roofline_launch_ms"] > 0 and rf["counters_scaled_by"] == 1.0 / world
