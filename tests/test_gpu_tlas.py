"""The top layer rebuilt on the device (atn_tlas_rebuild, csrc/device/tlas.hpp, docs/TLAS.md) against its CPU twin
(tests/cxx/tlas_oracle.cpp): every record field for field, the block path and the general path byte for byte, frames and
closest-hit records against the oracle walking the twin's layer and against the same context ticked with the host-built layer
(on the scenes tests/test_tlas_oracle_cpu.py cleared of ties), the skinned tick without a read-back, frames in flight, mixed
sequences, every shard of the node-wide renderer, and the refusals."""
import ctypes

import numpy as np
import pytest

import tlas_oracle as O
import tlas_scenes as T
from aten_amd import layout as L
from aten_amd.renderer import AtenAmdError
from aten_amd.scene.camera import create_camera
from test_gpu_lbvh import same_frame

pytestmark = pytest.mark.gpu

W, H = T.W, T.H
INVALID_ARG, NO_SCENE, UNSUPPORTED = -1, -4, -5
END = 0xffffffff


def context(fs, cam=None, fif=1, planar=None):
    from aten_amd.renderer import PathTracing
    r = PathTracing(0)
    try:
        if planar is not None:
            r.set_upload_options(planar_lights=planar)
        r.UpdateSceneData(fs)
        cam = cam or dict(pos=(0.0, 0.0, 14.0), at=(0.0, 0.0, 0.0), vfov=45.0)
        r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H))
        r.initSampler(W, H, 0)
        r.set_frames_in_flight(fif)
    except Exception:
        r.close()
        raise
    return r


def device_leaves(rec, root, base):
    """Walks device records along the hit links from the root link: {objid: record row} of the TLAS leaves, and the walk's length."""
    leaves, steps, link = {}, 0, root & END
    while link != END:
        i = ((link & O.LINK_OFFSET_MASK) - base) // 32
        assert 0 <= i < len(rec) and steps <= len(rec)
        steps += 1
        if link & O.LINK_NOT_INNER:
            assert link & O.LINK_TLAS_BIT
            assert int(rec[i, 0]) not in leaves
            leaves[int(rec[i, 0])] = rec[i].copy()
            link = int(rec[i, 5])
        else:
            link = int(rec[i, 3])
    return leaves, steps


def assert_records_equal_twin(rec, root, base, twin, objects, matrices, uploaded):
    """Every field of the device records against the twin's nodes.  The placement is the documented one: inner node i at record i,
    the leaf with table index k at record n - 1 + k."""
    table, nodes, idx = twin["table"], twin["nodes"], twin["indices"].astype(np.int64)
    n = len(table)
    assert len(rec) == 2 * n - 1 and root == base            # an inner root, first
    to_rec = np.concatenate([np.arange(n - 1), n - 1 + idx])        # twin node -> device record
    is_leaf = np.arange(2 * n - 1) >= n - 1

    def want_link(v):
        v = v.astype(np.int64)
        typed = (base + 32 * to_rec[np.maximum(v, 0)]) | np.where(is_leaf[np.maximum(v, 0)], O.LINK_NOT_INNER | O.LINK_TLAS_BIT, 0)
        return np.where(v < 0, END, typed).astype(np.uint32)
    hit, miss = want_link(nodes["hit"]), want_link(nodes["miss"])
    inner = rec[to_rec[:n - 1]]
    assert inner[:, 0:3].tobytes() == np.ascontiguousarray(nodes["boxmin"][:n - 1]).tobytes()
    assert inner[:, 4:7].tobytes() == np.ascontiguousarray(nodes["boxmax"][:n - 1]).tobytes()
    assert np.array_equal(inner[:, 3], hit[:n - 1]) and np.array_equal(inner[:, 7], miss[:n - 1])
    leaf = rec[to_rec[n - 1:]]
    objid = nodes["f0"][n - 1:].astype(np.int32)
    mtx_id = objects["mtx_id"][objid]
    w2l = np.where(mtx_id >= 0, 4 * (mtx_id + 1), -1).astype(np.int32)
    ident = np.array([m >= 0 and matrices[m + 1].tobytes() == np.eye(4, dtype=np.float32).tobytes() for m in mtx_id])
    assert np.array_equal(leaf[:, 0].view(np.int32), objid)
    assert np.array_equal(leaf[:, 1].view(np.int32), w2l)
    assert np.array_equal(leaf[:, 3].view(np.int32), ident.astype(np.int32))
    assert np.array_equal(leaf[:, 4].view(np.int32), nodes["f3"][n - 1:].astype(np.int32))
    assert np.array_equal(leaf[:, 5], hit[n - 1:]) and np.array_equal(leaf[:, 6], miss[n - 1:])
    assert np.array_equal(leaf[:, 5], leaf[:, 6])
    for row, o in zip(leaf, objid):                         # the list's root link and twin word: what the upload wrote for that object
        assert row[2] == uploaded[int(o)][2] and row[7] == uploaded[int(o)][7]
    got, steps = device_leaves(rec, root, base)
    assert steps == 2 * n - 1 and sorted(got) == sorted(objid.tolist())


# ---- 1. records against the twin -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [x for x in T.SIZES if x > 1])
def test_records_equal_the_twin(n):
    fs, inst = T.quad_instances(n)
    r = context(fs)
    try:
        uploaded, _ = device_leaves(*r.tlas_records())
        assert len(uploaded) == n
        table = O.leaf_table(fs.arrays["bvh_lists"][0])
        for tick in range(2):
            mtx = T.new_matrices(fs, inst, 10 * n + tick)
            r.tlas_rebuild(fs.arrays["objects"], mtx)
            twin = O.build(table, fs.arrays["objects"], mtx, O.local_boxes(fs, table))
            twin["table"] = table
            rec, root, base = r.tlas_records()
            assert_records_equal_twin(rec, root, base, twin, fs.arrays["objects"], mtx, uploaded)
            if n >= 3:
                assert int((rec[n - 1:, 3] == 1).sum()) == 1 and int((rec[n - 1:, 1].view(np.int32) == -1).sum()) == 1
        assert np.isfinite(r.render(W, H, frame=0)).all()
    finally:
        r.close()


@pytest.mark.parametrize("n", [2, 65, 1024])
def test_block_path_and_general_path_write_the_same_bytes(n):
    fs, inst = T.quad_instances(n)
    r = context(fs)
    try:
        mtx = T.new_matrices(fs, inst, n)
        r.tlas_rebuild(fs.arrays["objects"], mtx)
        a = r.tlas_records()
        r.tlas_rebuild(fs.arrays["objects"], T.new_matrices(fs, inst, n + 1), force_general=True)      # (other bytes in between)
        assert r.tlas_records()[0].tobytes() != a[0].tobytes()
        r.tlas_rebuild(fs.arrays["objects"], mtx, force_general=True)
        b = r.tlas_records()
        assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    finally:
        r.close()


def test_one_instance_is_written_from_the_host_and_keeps_the_direct_root():
    fs, inst = T.quad_instances(1)
    cam = dict(pos=(0.0, 0.0, 14.0), at=tuple(float(x) for x in fs.arrays["matrices"][0][:3, 3]), vfov=45.0)
    r = context(fs, cam)
    try:
        before_rec = r.tlas_records()
        before = r.render(W, H, frame=0).copy()
        assert before[..., :3].max() > 0
        r.tlas_rebuild()
        assert r.tlas_records()[0].tobytes() == before_rec[0].tobytes() and r.tlas_records()[1:] == before_rec[1:]
        assert before_rec[1] & O.LINK_TLAS_BIT and len(before_rec[0]) == 1        # the root link names the one leaf
        r.reset()
        assert r.render(W, H, frame=0).tobytes() == before.tobytes()
        r.tlas_rebuild(fs.arrays["objects"], fs.arrays["matrices"], force_general=True)
        r.reset()
        assert r.render(W, H, frame=0).tobytes() == before.tobytes()
    finally:
        r.close()


# ---- 2. frames -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rendered_scenes():
    return dict(cornell=T.cornell_ticks(), quad_room=T.quad_room_ticks())


@pytest.mark.parametrize("scene", ["cornell", "quad_room"])
def test_ticks_render_like_the_oracle_and_like_the_host_built_layer(orc, rendered_scenes, scene):
    ticks, cam = rendered_scenes[scene]
    c = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)
    seeds = orc.init_sampler(W, H, 0)
    r, host = context(ticks[0], cam), context(ticks[0], cam)
    try:
        for k, fs in enumerate(ticks[1:]):
            r.tlas_rebuild(fs.arrays["objects"], fs.arrays["matrices"])
            host.updateBVH(fs)
            r.reset()
            got = r.render(W, H, frame=k)
            rays = orc.generate_paths(c, seeds, W, H, 0, k)
            gi = r.trace_closest(rays)
            assert gi.tobytes() == host.trace_closest(rays).tobytes(), "tick %d" % k
            top = fs.arrays["bvh_lists"][0].copy()
            O.scene_with_twin_top(fs)
            try:
                assert gi.tobytes() == orc.trace_closest(fs, rays)[0].tobytes(), "tick %d" % k
                assert same_frame(got, orc.render(fs, c, seeds, W, H, frame=k)), "tick %d" % k
            finally:
                fs.replace_bvh_list(0, top)
        assert (gi["objid"] >= 0).sum() > 0.5 * W * H
    finally:
        r.close(); host.close()


# ---- 3. the whole tick on the device ---------------------------------------------------------------------------------------------
def test_skinned_tick_needs_no_box_from_the_host(orc):
    from test_gpu_skinning import N_BONES, Room
    room = Room(48, 24)
    d, cam = room.d, room.cam
    c = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)
    rays = orc.generate_paths(c, orc.init_sampler(W, H, 0), W, H, 0, 0)
    up = room.fs0.arrays["bvh_lists"][d["list"]][0]
    dev, back, stale = context(room.fs0, cam), context(room.fs0, cam), context(room.fs0, cam)
    try:
        skins = [x.skin_create(room.sv, d["v0"], d["t0"], d["n"], N_BONES) for x in (dev, back, stale)]
        differed = 0
        for k, t in enumerate(room.ticks):
            # the pose leaves the uploaded box: a top layer that kept it would cut the mesh
            assert (t["bbox"][:3] < up["boxmin"]).any() or (t["bbox"][3:] > up["boxmax"]).any()
            dev.skin_update(skins[0], t["palette"])
            assert dev.skin_compute(skins[0], t["restart"], want_bbox=False) is None
            dev.lbvh_rebuild_list_skinned(d["list"], skins[0])
            dev.tlas_rebuild()
            back.skin_update(skins[1], t["palette"])
            mn, mx = back.skin_compute(skins[1], t["restart"])
            back.lbvh_rebuild_list(d["list"], d["t0"], d["n"], mn, mx)
            back.updateBVH(t["fs"])
            stale.skin_update(skins[2], t["palette"])
            stale.skin_compute(skins[2], t["restart"], want_bbox=False)
            stale.lbvh_rebuild_list_skinned(d["list"], skins[2])
            for x in (dev, back, stale):
                x.reset()
            a, b, s = (x.render(W, H, frame=k).copy() for x in (dev, back, stale))
            assert same_frame(a, b), "tick %d" % k
            gi = dev.trace_closest(rays)
            assert gi.tobytes() == back.trace_closest(rays).tobytes(), "tick %d" % k
            differed += int(stale.trace_closest(rays).tobytes() != gi.tobytes() and s.tobytes() != a.tobytes())
        assert differed >= 1            # without the rebuild the part that moved is cut off
        assert (gi["objid"] == len(room.fs0.arrays["objects"]) - 1).sum() > 300
    finally:
        dev.close(); back.close(); stale.close()


# ---- 4. frames in flight ---------------------------------------------------------------------------------------------------------
def test_frames_in_flight_do_not_show_in_the_films(rendered_scenes):
    ticks, cam = rendered_scenes["cornell"]

    def run(fif):
        r = context(ticks[0], cam, fif)
        films = []
        try:
            f = 0
            for rep in range(2):
                for fs in ticks[1:]:
                    r.tlas_rebuild(fs.arrays["objects"], fs.arrays["matrices"])
                    for _ in range(2):
                        r.render(W, H, frame=f, download=False); f += 1
                    if rep:
                        r.tlas_rebuild()                                            # (twice in a tick, without arguments)
                films.append(r.download_film().copy())
            return films
        finally:
            r.close()
    a, b = run(1), run(3)
    assert len(a) == 2 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert (a[-1][..., 3] == 12).all()


def test_frames_in_flight_n_to_1_to_n_keeps_scene_sets_current(orc, rendered_scenes):
    ticks, cam = rendered_scenes["quad_room"]
    c = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)
    rays = orc.generate_paths(c, orc.init_sampler(W, H, 0), W, H, 0, 0)
    r, host = context(ticks[0], cam), context(ticks[0], cam)
    try:
        f = 0
        for nfl, seq in [(3, [1, 2, 3, 1]), (1, [2]), (3, [3, 1]), (1, [2, 3]), (2, [1, 2, 3])]:
            r.set_frames_in_flight(nfl)
            for k in seq:
                fs = ticks[k]
                if f % 2:
                    r.tlas_rebuild(fs.arrays["objects"], fs.arrays["matrices"])
                else:                                   # the matrices first, the layer in a call of its own
                    r.updateBVH(fs)
                    r.tlas_rebuild()
                r.render(W, H, frame=f, download=False); f += 1
            host.updateBVH(ticks[seq[-1]])
            assert r.trace_closest(rays).tobytes() == host.trace_closest(rays).tobytes(), "after the phase with %d frame(s) in flight" % nfl
    finally:
        r.close(); host.close()


# ---- 5. mixed sequences ----------------------------------------------------------------------------------------------------------
def test_update_tlas_and_tlas_rebuild_alternate(orc, rendered_scenes):
    ticks, cam = rendered_scenes["cornell"]
    c = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)
    rays = orc.generate_paths(c, orc.init_sampler(W, H, 0), W, H, 0, 0)
    r, host = context(ticks[0], cam), context(ticks[0], cam)
    try:
        for step, k in enumerate([1, 2, 3, 1, 2, 3]):
            fs = ticks[k]
            if step % 2:
                r.updateBVH(fs)
            else:
                r.tlas_rebuild(fs.arrays["objects"], fs.arrays["matrices"])
            host.updateBVH(fs)
            assert r.trace_closest(rays).tobytes() == host.trace_closest(rays).tobytes(), "step %d" % step
            assert len(r.tlas_records()[0]) == (len(fs.arrays["bvh_lists"][0]) if step % 2 else 2 * len(O.leaf_table(fs.arrays["bvh_lists"][0])) - 1)
    finally:
        r.close(); host.close()


def test_planar_light_flags_follow_the_lamp(rendered_scenes):
    """The lamp's records come back unchanged: the flag stays.  The lamp's matrix moves: the flag goes.  The films do not depend on
    the flag: a context uploaded without planar lights renders the same bytes."""
    ticks, cam = rendered_scenes["cornell"]
    fs = ticks[1]
    a = fs.arrays
    lamp = int(a["lights"][0]["arealight_objid"])
    moved = a["matrices"].copy()
    mid = int(a["objects"][lamp]["mtx_id"])
    moved[mid, 1, 3] -= 0.125; moved[mid + 1, 1, 3] += 0.125
    r, plain = context(ticks[0], cam), context(ticks[0], cam, planar=0)
    try:
        assert r.planar_area_lights() == 1 and plain.planar_area_lights() == 0
        for x in (r, plain):
            x.tlas_rebuild(a["objects"], a["matrices"])
            x.reset()
        assert r.planar_area_lights() == 1
        assert r.render(W, H, frame=0).tobytes() == plain.render(W, H, frame=0).tobytes()
        for x in (r, plain):
            x.tlas_rebuild(matrices=moved)
            x.reset()
        assert r.planar_area_lights() == 0
        assert r.render(W, H, frame=1).tobytes() == plain.render(W, H, frame=1).tobytes()
    finally:
        r.close(); plain.close()


def test_every_walk_flavour_reads_the_rebuilt_layer_alike(rendered_scenes, monkeypatch):
    ticks, cam = rendered_scenes["cornell"]
    films = []
    for env in ({}, {"ATEN_AMD_LDS_NODES": "0"}, {"ATEN_AMD_TRACE": "r"}, {"ATEN_AMD_TRACE": "s"}):
        for k in ("ATEN_AMD_LDS_NODES", "ATEN_AMD_TRACE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)            # (read once, when the context is created)
        r = context(ticks[0], cam)
        try:
            for fs in ticks[1:3]:
                r.tlas_rebuild(fs.arrays["objects"], fs.arrays["matrices"])
                r.render(W, H, frame=len(films), download=False)
            r.reset()
            films.append(r.render(W, H, frame=3).copy())
        finally:
            r.close()
    assert all(f.tobytes() == films[0].tobytes() for f in films[1:])
    assert films[0][..., :3].max() > 0


def test_shards_equal_one_context(rendered_scenes):
    from aten_amd.renderer import MultiGpuPathTracing
    ticks, cam = rendered_scenes["cornell"]
    c = create_camera(cam["pos"], cam["at"], cam["vfov"], W, H)
    r = context(ticks[0], cam)
    mg = MultiGpuPathTracing([0, 0, 0])
    try:
        mg.UpdateSceneData(ticks[0]); mg.updateCamera(c); mg.initSampler(W, H, 0)
        for k, fs in enumerate(ticks[1:]):
            for x in (r, mg):
                x.tlas_rebuild(fs.arrays["objects"], fs.arrays["matrices"], force_general=bool(k % 2))
                x.reset()
            assert mg.render(W, H, frame=k).tobytes() == r.render(W, H, frame=k).tobytes()
    finally:
        r.close(); mg.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_scene_as_it_was(rendered_scenes):
    from aten_amd.renderer import PathTracing
    ticks, cam = rendered_scenes["cornell"]
    fs = ticks[1]
    a = fs.arrays
    empty = PathTracing(0)
    try:
        assert empty._l.atn_tlas_rebuild(empty._ctx, None, 0, None, 0, 0) == NO_SCENE
        with pytest.raises(AtenAmdError, match="atn_upload_scene"):
            empty.tlas_rebuild()
        with pytest.raises(AtenAmdError, match="atn_upload_scene"):
            empty.tlas_records()
    finally:
        empty.close()
    r = context(ticks[0], cam)
    try:
        r.tlas_rebuild(a["objects"], a["matrices"])
        before = r.render(W, H, frame=0).copy()
        rec = r.tlas_records()
        objs = np.ascontiguousarray(a["objects"]); mtx = np.ascontiguousarray(a["matrices"])

        def refused(code, pattern, o, no, m, nm):
            assert r._l.atn_tlas_rebuild(r._ctx, o, no, m, nm, 0) == code
            assert pattern in r._l.atn_last_error(r._ctx).decode()
        refused(INVALID_ARG, "do not match", None, len(objs), None, 0)
        refused(INVALID_ARG, "do not match", objs.ctypes.data, 0, None, 0)
        refused(INVALID_ARG, "null matrix", None, 0, None, len(mtx))
        bad = objs.copy(); bad["mtx_id"][-1] = len(mtx)
        refused(UNSUPPORTED, "matrix index out of range", bad.ctypes.data, len(bad), None, 0)
        refused(UNSUPPORTED, "matrix index out of range", None, 0, mtx.ctypes.data, 2)            # the kept objects against fewer matrices
        bad = objs.copy(); bad["light_id"][-1] = 7
        refused(UNSUPPORTED, "light id out of range", bad.ctypes.data, len(bad), None, 0)
        bad = objs.copy(); bad["object_id"][-1] = len(objs)
        refused(UNSUPPORTED, "object id out of range", bad.ctypes.data, len(bad), None, 0)
        refused(UNSUPPORTED, "leaf object id out of range", objs.ctypes.data, len(objs) - 1, None, 0)  # fewer objects than a leaf names
        assert r._l.atn_tlas_download(r._ctx, np.zeros(8, np.uint32).ctypes.data, 32, ctypes.c_uint32(0), None, None) == INVALID_ARG
        r.reset()
        assert r.render(W, H, frame=0).tobytes() == before.tobytes()
        now = r.tlas_records()
        assert now[0].tobytes() == rec[0].tobytes() and now[1:] == rec[1:]
        # a top layer without an instance leaf: one leaf with neither triangle nor nested tree
        dead = np.zeros(1, L.BVH_NODE)
        dead["hit"] = dead["miss"] = -1; dead["f0"] = 0; dead["f1"] = dead["f2"] = dead["f3"] = -1
        assert r._l.atn_update_tlas(r._ctx, objs.ctypes.data, len(objs), None, 0, dead.ctypes.data, 1) == 0
        r.reset()
        black = r.render(W, H, frame=0).copy()
        refused(UNSUPPORTED, "no instance leaf", None, 0, None, 0)
        r.reset()
        assert r.render(W, H, frame=0).tobytes() == black.tobytes() and black.tobytes() != before.tobytes()
        r.updateBVH(fs)                                     # a host-given layer brings the leaves back
        r.tlas_rebuild()
        r.reset()
        assert r.render(W, H, frame=0).tobytes() == before.tobytes()
    finally:
        r.close()

