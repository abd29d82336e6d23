"""Geometry motion vectors on the CPU: the twin (tests/cxx/motion_oracle.cpp) against mathematics, the moved-quad scene through the
CPU oracle's SVGF (the newly covered strip keeps its history with the twin's plane and loses it with the static one), and the
library's new entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

import motion_oracle as M
from motion_oracle import MARGIN_ROWS, SHIFT_COLUMNS, counted_strip, ids_of, quad_rooms
from aten_amd import layout as L
from conftest import make_camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atn_set_geometry_motion", "atn_geometry_motion_stats", "atn_geometry_motion_matrices")
W, H = 96, 64


@pytest.fixture(scope="module")
def quad(orc):
    """The two quad scenes, the oracle's primary hits of frame 0 (before) and frame 1 (after), and their ids planes."""
    fs0, fs1, cam, info = quad_rooms()
    c = make_camera(orc, cam, W, H)
    seeds = orc.init_sampler(W, H, 0)
    hits = [orc.trace_closest(fs, orc.generate_paths(c, seeds, W, H, 0, frame))[0] for frame, fs in ((0, fs0), (1, fs1))]
    return dict(fs=(fs0, fs1), cam=cam, c=c, seeds=seeds, info=info, ids=[ids_of(x, W, H) for x in hits])


def twin_plane(fs_now, fs_before, ids, w2c, prev_w2c):
    a, b = fs_now.arrays, fs_before.arrays
    return M.motion_geometry(ids, a["objects"], a["triangles"], a["vtx_pos"], b["vtx_pos"], a["matrices"], b["matrices"], w2c, prev_w2c)


# ---- 1. symbols -------------------------------------------------------------------------------------------------------------------
def test_library_exports_geometry_motion_entry_points():
    from aten_amd import _lib
    so = os.environ.get("ATEN_AMD_LIB") or os.path.join(ROOT, "aten_amd", "libaten_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    for s in NAMES:
        assert s in _lib.SYMBOLS
        assert s in names, s
        assert re.search(r"^int %s\(atn_ctx\* ctx" % s, header, re.M), s
    assert L.OBJECT_PARAM.itemsize == M.lib().orc_motion_sizeof_object()


# ---- 2. the twin against mathematics ----------------------------------------------------------------------------------------------
def test_history_equal_to_the_scene_gives_the_static_formula(quad):
    """With H equal to the scene the twin is motion_depth over its own current positions, bit for bit -- also under a camera move."""
    fs = quad["fs"][1]
    ids = quad["ids"][1]
    aspect = W / H
    w2c = M.world_to_clip(quad["cam"]["pos"], quad["cam"]["at"], quad["cam"]["vfov"], aspect)
    moved = M.world_to_clip((0.3, 1.1, 2.9), (0.05, 0.95, 0.0), quad["cam"]["vfov"], aspect)
    for prev in (w2c, moved):
        md, pos = twin_plane(fs, fs, ids, w2c, prev)
        want = M.motion_static(pos, w2c, prev)
        assert np.array_equal(md.view(np.uint32), want.view(np.uint32))
        hit = ids[..., 0].copy().view(np.int32) >= 0
        assert hit.any() and (~hit).any()
        assert np.all(md[~hit] == np.array([0, 0, -1, 1], np.float32)) and np.all(pos[~hit] == 0) and np.all(pos[hit][:, 3] == 1)
        if prev is w2c:
            assert np.all(md[hit][:, :2] == 0)
        else:
            assert np.count_nonzero(md[hit][:, :2]) > hit.sum()


def test_translated_instance_against_float64(quad):
    """A pure translation of the quad's instance: motion.xy against the projection difference in float64 (from the same float32
    inputs), within 4 ulp of the larger of the two screen coordinates it is the difference of."""
    fs0, fs1 = quad["fs"]
    ids = quad["ids"][1]
    w2c = M.world_to_clip(quad["cam"]["pos"], quad["cam"]["at"], quad["cam"]["vfov"], W / H)
    md, _ = twin_plane(fs1, fs0, ids, w2c, w2c)
    oid = ids[..., 0].copy().view(np.int32)
    on_quad = oid == quad["info"]["instance"]
    assert on_quad.sum() > 100
    a = fs1.arrays
    tri = a["triangles"][ids[..., 1].copy().view(np.int32)[on_quad]]
    v = a["vtx_pos"].astype(np.float64)
    ba, bb = ids[..., 2][on_quad].astype(np.float64), ids[..., 3][on_quad].astype(np.float64)
    local = ((1 - ba - bb)[:, None] * v[tri["idx"][:, 0], :3] + ba[:, None] * v[tri["idx"][:, 1], :3] + bb[:, None] * v[tri["idx"][:, 2], :3])
    m = w2c.astype(np.float64)

    def screen(mat):
        p = np.concatenate([local, np.ones((len(local), 1))], 1) @ mat.astype(np.float64).T
        clip = p @ m.T
        return clip[:, :2] / clip[:, 3:4] * 0.5 + 0.5
    mid = quad["info"]["mtx_id"]
    cur, prv = screen(a["matrices"][mid]), screen(fs0.arrays["matrices"][mid])
    want = prv - cur
    assert np.all(np.abs(want[:, 0]) > 3.0 / W) and np.all(want[:, 1] == 0)        # the quad moved by s columns, along x only
    larger = np.maximum(np.abs(cur), np.abs(prv)).astype(np.float32)
    err = np.abs(md[on_quad][:, :2].astype(np.float64) - want)
    assert np.all(err <= 4 * np.spacing(larger).astype(np.float64)), float((err / np.spacing(larger)).max())
    # everything else stood still under an unmoved camera
    still = (oid >= 0) & ~on_quad
    assert np.all(md[still][:, :2] == 0)


def test_a_moved_vertex_changes_only_its_triangles(quad):
    fs = quad["fs"][1]
    ids = quad["ids"][1]
    a = fs.arrays
    w2c = M.world_to_clip(quad["cam"]["pos"], quad["cam"]["at"], quad["cam"]["vfov"], W / H)
    base, _ = twin_plane(fs, fs, ids, w2c, w2c)
    oid, tid = ids[..., 0].copy().view(np.int32), ids[..., 1].copy().view(np.int32)
    # a vertex of the triangle most pixels see
    seen = tid[oid >= 0]
    t = np.bincount(seen).argmax()
    vi = int(a["triangles"][t]["idx"][1])
    hv = a["vtx_pos"].copy()
    hv[vi, :3] += np.array([0.05, -0.03, 0.02], np.float32)
    md, _ = M.motion_geometry(ids, a["objects"], a["triangles"], a["vtx_pos"], hv, a["matrices"], a["matrices"], w2c, w2c)
    uses = (a["triangles"]["idx"] == vi).any(1)
    on = (oid >= 0) & uses[np.where(oid >= 0, tid, 0)]
    changed = (md.view(np.uint32) != base.view(np.uint32)).any(-1)
    assert on.any() and changed.any()
    assert not np.any(changed & ~on)
    # (a pixel whose barycentric weight of that vertex is 0 may stay; the others move)
    assert changed[on].mean() > 0.9


# ---- 3. the newly covered strip keeps its history -------------------------------------------------------------------------------
def test_strip_keeps_history_with_the_twins_plane_and_loses_it_with_the_static_one(orc, quad):
    fs0, fs1 = quad["fs"]
    c, seeds = quad["c"], quad["seeds"]
    inst = quad["info"]["instance"]
    before = quad["ids"][0][..., 0].copy().view(np.int32) == inst
    after = quad["ids"][1][..., 0].copy().view(np.int32) == inst
    counted = counted_strip(before, after)
    assert counted.any(1).sum() == after.any(1).sum() - 2 * MARGIN_ROWS >= 6         # every row inside the quad has counted pixels
    w2c = M.world_to_clip(quad["cam"]["pos"], quad["cam"]["at"], quad["cam"]["vfov"], W / H)
    plane, _ = twin_plane(fs1, fs0, quad["ids"][1], w2c, w2c)
    # the vector points back by s columns on the quad and nowhere else
    assert np.allclose(plane[after][:, 0] * W, -SHIFT_COLUMNS, atol=1e-3) and np.all(plane[..., 1] == 0)
    weights = {}
    for kind in ("twin", "static"):
        sv = orc.Svgf()
        try:
            sv.render(fs0, c, seeds, W, H, 3, 3, frame=0, compute_motion=True)
            if kind == "twin":
                sv.set_motion_depth(plane)
            sv.render(fs1, c, seeds, W, H, 3, 3, frame=1, compute_motion=kind == "static")
            if kind == "static":
                assert np.all(sv.buffer("motion_depth")[..., :2] == 0)
            weights[kind] = sv.buffer("prev_moment_temporalweight")[..., 3].copy()
        finally:
            sv.close()
    assert np.all(weights["twin"][counted] > 0)
    assert np.all(weights["static"][counted] == 0)
