"""The CPU twin of the device-built top layer (tests/cxx/tlas_oracle.cpp, docs/TLAS.md), without a GPU:

  * the structure of the twin's tree for every size the GPU tests use and for two degenerate sets;
  * the SCENE CONDITION of the GPU tests: through the host-built top layer and through the twin's, the oracle's closest-hit walk
    returns byte-identical records for the primary rays and the bounce-1 rays of a frame -- two different trees visit the instances
    in different orders, so a scene with coincident surfaces in two instances would let tie-breaking decide; such a scene is not
    used (zero rays may differ: the assertion is the condition, not a tolerance);
  * the twin as a stand-alone program under AddressSanitizer and UBSan.
"""
import os
import subprocess

import numpy as np
import pytest

import tlas_oracle as O
import tlas_scenes as T
from aten_amd import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def walk(nodes):
    order, i = [], 0
    while i >= 0:
        order.append(i)
        i = int(nodes[i]["hit"])
    return order


def check_structure(t, n):
    nodes = t["nodes"]
    assert len(nodes) == 2 * n - 1
    assert O.check(nodes, n) == 0
    # the same rules once more, in numpy: every leaf exactly once along the hit links, links forward
    order = walk(nodes)
    assert sorted(order) == list(range(2 * n - 1))
    pos = np.empty(2 * n - 1, np.int64); pos[order] = np.arange(2 * n - 1)
    leaf = (nodes["f0"] >= 0) | (nodes["f1"] >= 0)
    assert int(leaf.sum()) == n and sorted(nodes["f0"][leaf].astype(int)) == sorted(t["table"][:, 0].astype(int))
    for k in ("hit", "miss"):
        l = nodes[k].astype(np.int64)
        assert ((l < 0) | (pos[np.maximum(l, 0)] > pos)).all()
    # sorted by code, equal codes in table order
    c, i = t["codes"].astype(np.int64), t["indices"].astype(np.int64)
    assert ((np.diff(c) > 0) | ((np.diff(c) == 0) & (np.diff(i) > 0))).all()
    assert sorted(i) == list(range(n))


@pytest.mark.parametrize("n", T.SIZES)
def test_twin_tree_structure(n):
    fs, inst = T.quad_instances(n)
    table = O.leaf_table(fs.arrays["bvh_lists"][0])
    assert len(table) == n
    t = O.build(table, fs.arrays["objects"], T.new_matrices(fs, inst, 5), O.local_boxes(fs, table))
    t["table"] = table
    check_structure(t, n)
    if n >= 3:      # the instance without a matrix keeps the mesh's own box
        k = list(O.table_objids(table)).index(inst[1])
        assert t["world"][k].tobytes() == np.float32([-0.5, -0.5, 0, 0.5, 0.5, 0]).tobytes()


@pytest.mark.parametrize("kind", ["identical", "planar"])
def test_twin_tree_structure_degenerate(kind):
    objs, mtx, table, boxes = T.degenerate_instances(kind)
    t = O.build(table, objs, mtx, boxes)
    t["table"] = table
    check_structure(t, len(table))
    if kind == "identical":
        assert len(np.unique(t["codes"])) == 1 and ((t["codes"] & 0x09249249) == 0).all()       # the flat z axis: coordinate 0 by the select
        assert np.array_equal(t["indices"], np.arange(len(table)))              # ... and the sort keeps the table's order
    else:
        assert ((t["codes"] & 0x09249249) == 0).all() and len(np.unique(t["codes"])) > 100      # the z bits only


def bounce_rays(orc, fs, cam, seeds, bounce):
    rec, b, _ = orc.record_vertices(fs, cam, seeds, T.W, T.H, frame=0)
    r = np.zeros(int((b == bounce).sum()), L.RAY)
    r["org"], r["dir"] = rec["org"][b == bounce], rec["dir"][b == bounce]
    return r


@pytest.mark.parametrize("scene", ["cornell", "quad_room", "skinned_room"])
def test_scene_has_no_tie_between_the_two_top_layers(orc, scene):
    if scene == "skinned_room":         # the ticks as the host skins them: the tube's list is the host's tree over the skinned vertices
        from test_gpu_skinning import Room
        room = Room(48, 24)
        ticks, cam = [room.fs0] + [t["fs"] for t in room.ticks], room.cam
    else:
        ticks, cam = T.cornell_ticks() if scene == "cornell" else T.quad_room_ticks()
    c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], T.W, T.H)
    seeds = orc.init_sampler(T.W, T.H, 0)
    for k, fs in enumerate(ticks[1:]):
        rays = [orc.generate_paths(c, seeds, T.W, T.H, 0, 0), bounce_rays(orc, fs, c, seeds, 1)]
        assert len(rays[1]) > 1000
        host = [orc.trace_closest(fs, r)[0] for r in rays]
        t = O.scene_with_twin_top(fs)
        assert O.check(t["nodes"], len(t["table"])) == 0
        for r, h in zip(rays, host):
            assert orc.trace_closest(fs, r)[0].tobytes() == h.tobytes(), "tick %d" % k


def test_the_twin_runs_clean_under_asan_and_ubsan_in_a_program_of_its_own(tmp_path):
    exe = str(tmp_path / "tlas_oracle_san")
    subprocess.check_call(["g++"] + O.CXXFLAGS + ["-g", "-DTLAS_ORACLE_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                  "-o", exe, O.SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
