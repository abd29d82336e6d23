"""Geometry motion vectors on the device (atn_set_geometry_motion, compute_motion = 2; csrc/device/motion.hpp, docs/MOTION.md) against
their CPU twin (tests/cxx/motion_oracle.cpp) on a moved instance and on a skinned mesh, and through SVGF and ReSTIR."""
import numpy as np
import pytest

import motion_oracle as M
import skinning_oracle as S
from aten_amd.renderer import AtenAmdError, PathTracing, unpack_primary_hit
from aten_amd.scene.camera import create_camera
from conftest import parity_record
from motion_oracle import MARGIN_ROWS, SHIFT_COLUMNS, column_width, counted_strip, quad_rooms

pytestmark = pytest.mark.gpu

N_BONES = 8
INVALID_ARG, UNSUPPORTED = -1, -5
SIZES = [(100, 52), (96, 64)]       # a width that is no multiple of 8 with a height that is no multiple of 32, and the strip test's frame
DEPTH = 3


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def new_context(fs, cam, w, h, fif=1, motion=True):
    r = PathTracing(0)
    try:
        r.UpdateSceneData(fs)
        r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], w, h))
        r.initSampler(w, h, 0)
        r.set_frames_in_flight(fif)
        if motion:
            r.set_geometry_motion(True)
    except Exception:
        r.close()
        raise
    return r


def status_of(call):
    with pytest.raises(AtenAmdError) as e:
        call()
    return int(str(e.value).rsplit("(status ", 1)[1].rstrip(")"))


def host_scene(fs):
    a = fs.arrays
    return dict(objects=a["objects"], triangles=a["triangles"], vtx=a["vtx_pos"].copy(), mtx=a["matrices"].copy())


def twin_of_frame(r, ids, now, hist):
    """The twin's (motion plane, positions) for the frame the context just rendered: its ids, the scene it read, the history."""
    w2c, prev = r.geometry_motion_matrices()
    return M.motion_geometry(ids, now["objects"], now["triangles"], now["vtx"], hist["vtx"], now["mtx"], hist["mtx"], w2c, prev)


def check_plane(config, got, want):
    """Bit for bit; where a last bit differs the bound of the static pass (tests/test_gpu_svgf.py): every pixel within 1e-5."""
    m = parity_record(config, got, want, tol=1e-5)
    if not np.array_equal(bits(got), bits(want)):
        assert m["frac_within_1e-05"] == 1.0 and np.array_equal(got[..., 3], want[..., 3]), m


class Skinned:
    """skinned_room(12, 6) and its first ticks as the host computes them (the top layer is the caller's business)."""

    def __init__(self, n_ticks=4):
        from aten_amd.scene import scenedefs
        self.b, self.oid, self.cam, self.sv = scenedefs.skinned_room(12, 6, N_BONES)
        self.fs0 = self.b.build()
        o = self.fs0.arrays["objects"][self.oid]
        self.t0, self.n = int(o["triangle_id"]), int(o["triangle_num"])
        tr = self.fs0.arrays["triangles"][self.t0:self.t0 + self.n]
        self.v0 = int(tr["idx"].min())
        self.list = self.fs0.blas_index[self.oid]
        self.nv, self.nt = len(self.fs0.arrays["vtx_pos"]), len(self.fs0.arrays["triangles"])
        twin = S.SkinTwin(self.sv, tr, vtx_offset=self.v0)
        self.ticks = []
        for k in range(n_ticks):
            pal = scenedefs.skinned_pose(0.9 * k + 0.4, N_BONES)
            twin.compute(pal, k == 0)
            self.b.set_mesh_vertices(self.oid, twin.pos[:, :3], np.arange(len(self.sv)).reshape(-1, 3), twin.nml[:, :3])
            self.ticks.append(dict(palette=pal, restart=k == 0, fs=self.b.build()))
        self.skin_tris = np.zeros(self.nt, bool)
        self.skin_tris[self.t0:self.t0 + self.n] = True

    def create_skin(self, r):
        return r.skin_create(self.sv, self.v0, self.t0, self.n, N_BONES)

    def tick(self, r, skin, k):
        t = self.ticks[k]
        r.skin_update(skin, t["palette"])
        assert r.skin_compute(skin, t["restart"], want_bbox=False) is None
        r.lbvh_rebuild_list_skinned(self.list, skin)
        r.updateBVH(t["fs"])

    def device_scene(self, r, skin, fs):
        d = r.skin_scene_arrays(skin, self.nv, self.nt)
        return dict(objects=fs.arrays["objects"], triangles=d["triangles"], vtx=d["vtx_pos"], mtx=fs.arrays["matrices"].copy())


@pytest.fixture(scope="module")
def skinned():
    return Skinned()


@pytest.fixture(scope="module")
def quads():
    return quad_rooms()


# ---- 1. the ids plane ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_primary_hit_is_the_frames_closest_hit_and_rebuilds_the_position(quads, w, h):
    fs0, fs1, cam, info = quads
    r = new_context(fs1, cam, w, h)
    try:
        now = host_scene(fs1)
        for frame, restir in ((0, False), (1, False), (2, True)):
            if restir:
                r.restir_render(w, h, DEPTH, 3, frame=frame, compute_motion=2)
                plane = r.restir_buffer("primary_hit")
                info_p = r.restir_buffer("info")
                pos, hit_flag = info_p["p"], info_p["hit"] == 1.0
            else:
                r.svgf_render(w, h, DEPTH, 3, spp=1, frame=frame, compute_motion=2)
                plane = r.svgf_buffer("primary_hit")
                pp = r.svgf_buffer("primary_position")
                pos, hit_flag = pp[..., :3], pp[..., 3] == 1.0
            ids = unpack_primary_hit(plane)
            want = r.trace_closest(r.generate_paths(w, h, sample=0, frame=frame)).reshape(h, w)
            hit = want["objid"] >= 0
            assert hit.any() and (~hit).any()
            assert np.array_equal(ids["objid"] >= 0, hit) and np.all(ids["objid"][~hit] == -1)
            assert np.array_equal(hit_flag, hit)
            for k, f in (("objid", "objid"), ("tri", "tri_id")):
                assert np.array_equal(ids[k][hit], want[f][hit]), k
            for k in ("a", "b"):
                assert np.array_equal(bits(ids[k][hit]), bits(want[k][hit])), k
            _, twin_pos = twin_of_frame(r, plane, now, now)
            assert np.array_equal(bits(twin_pos[..., :3][hit]), bits(pos[hit]))
    finally:
        r.close()


# ---- 2. nothing moved: mode 2 is mode 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,w,h", [("skinned", 100, 52), ("quad", 96, 64)])
def test_nothing_moved_equals_the_static_pass_byte_for_byte(skinned, quads, scene, w, h):
    fs, cam = (skinned.fs0, skinned.cam) if scene == "skinned" else (quads[0], quads[2])
    a, b = new_context(fs, cam, w, h, motion=False), new_context(fs, cam, w, h)
    try:
        for frame in range(3):
            if frame == 2:      # a camera move
                c2 = create_camera((0.2, 1.1, 2.9), (0.05, 0.95, 0.0), cam["vfov"], w, h)
                a.updateCamera(c2); b.updateCamera(c2)
            oa = a.svgf_render(w, h, DEPTH, 3, frame=frame, compute_motion=1)
            ob = b.svgf_render(w, h, DEPTH, 3, frame=frame, compute_motion=2)
            ma, mb = a.svgf_buffer("motion_depth"), b.svgf_buffer("motion_depth")
            assert np.array_equal(bits(ma), bits(mb)), frame
            assert np.array_equal(bits(oa), bits(ob)), frame
            if frame == 2:
                assert np.count_nonzero(mb[..., :2]) > 0
            ra = a.restir_render(w, h, DEPTH, 3, frame=frame, compute_motion=1)
            rb = b.restir_render(w, h, DEPTH, 3, frame=frame, compute_motion=2)
            assert np.array_equal(bits(a.restir_buffer("motion")), bits(b.restir_buffer("motion"))), frame
            assert np.array_equal(bits(ra), bits(rb)), frame
        assert b.geometry_motion_stats() == dict(passes=6, copies=0, copied_float4=0)     # no update: nothing copied
    finally:
        a.close(); b.close()


# ---- 3. a moved instance, skinned ticks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_moved_instance_equals_the_twin(w, h):
    from aten_amd.scene import scenedefs
    fs0, cam, info = scenedefs.moving_quad_room(0.0)
    step = column_width(cam, w, h, scenedefs.MOVING_QUAD["centre"][2])
    scenes = [fs0, scenedefs.moving_quad_room(5.3 * step)[0], scenedefs.moving_quad_room(-2.6 * step)[0]]
    r = new_context(fs0, cam, w, h)
    try:
        hist = host_scene(fs0)
        for k, fs in enumerate(scenes):
            if k:
                r.updateBVH(fs)         # (atn_update_tlas: objects, matrices, top layer)
            now = host_scene(fs)
            for restir in (False, True):
                if restir:
                    r.restir_render(w, h, DEPTH, 3, frame=2 * k + 1, compute_motion=2)
                    got, plane = r.restir_buffer("motion"), r.restir_buffer("primary_hit")
                else:
                    r.svgf_render(w, h, DEPTH, 3, frame=2 * k, compute_motion=2)
                    got, plane = r.svgf_buffer("motion_depth"), r.svgf_buffer("primary_hit")
                want, _ = twin_of_frame(r, plane, now, hist)
                check_plane("motion_quad_%dx%d_step%d_%s" % (w, h, k, "restir" if restir else "svgf"), got, want)
                ids = unpack_primary_hit(plane)
                on_quad = ids["objid"] == info["instance"]
                still = (ids["objid"] >= 0) & ~on_quad
                assert on_quad.sum() > 50
                if k:       # (a renderer's first frame has no previous camera: its previous matrix is the identity)
                    assert np.all(got[still][:, :2] == 0)                           # unmoved geometry under an unmoved camera: exactly 0
                    if restir:
                        assert np.all(got[on_quad][:, :2] == 0)                     # the SVGF frame in front of it saw the same scene
                    else:
                        moved_by = (5.3, -2.6 - 5.3)[k - 1]
                        assert np.allclose(got[on_quad][:, 0] * w, -moved_by, atol=1e-3) and np.all(got[on_quad][:, 1] == 0)
                hist = now
        st = r.geometry_motion_stats()
        assert st["passes"] == 6 and st["copies"] == 2 and st["copied_float4"] == 2 * 4 * len(fs0.arrays["matrices"])
    finally:
        r.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_skinned_ticks_equal_the_twin(skinned, w, h):
    r = new_context(skinned.fs0, skinned.cam, w, h)
    try:
        skin = skinned.create_skin(r)
        hist = skinned.device_scene(r, skin, skinned.fs0)
        r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=2)
        for k in range(3):
            skinned.tick(r, skin, k)
            now = skinned.device_scene(r, skin, skinned.ticks[k]["fs"])
            r.svgf_render(w, h, DEPTH, 3, frame=k + 1, compute_motion=2)
            got, plane = r.svgf_buffer("motion_depth"), r.svgf_buffer("primary_hit")
            want, _ = twin_of_frame(r, plane, now, hist)
            check_plane("motion_skinned_%dx%d_tick%d" % (w, h, k), got, want)
            ids = unpack_primary_hit(plane)
            hit = ids["objid"] >= 0
            on_skin = hit & skinned.skin_tris[np.where(hit, ids["tri"], 0)]
            assert on_skin.sum() > 20 and np.count_nonzero(got[on_skin][:, :2]) > on_skin.sum() // 2
            assert np.all(got[hit & ~on_skin][:, :2] == 0)
            hist = now
        # a tick copies the skin's vertex range and the matrices atn_update_tlas wrote, nothing else
        st = r.geometry_motion_stats()
        n_mtx = 4 * len(skinned.fs0.arrays["matrices"])
        assert st["passes"] == 4 and st["copies"] == 6 and st["copied_float4"] == 3 * (len(skinned.sv) + n_mtx)
    finally:
        r.close()


@pytest.mark.parametrize("fif", [1, 3])
def test_another_number_of_matrices_gives_zero_object_motion_for_one_frame(fif):
    """An instance is added between two mode-2 frames: the history's matrices are made equal to the scene's before the motion pass,
    so nothing moves on that frame (the first quad did move), and the frame after it follows the instances again."""
    from aten_amd.scene import scenedefs
    w, h = SIZES[0]
    fs0, cam, info = scenedefs.moving_quad_room(0.0)
    step = column_width(cam, w, h, scenedefs.MOVING_QUAD["centre"][2])
    fs1 = scenedefs.moving_quad_room(4.0 * step, second_offset=0.5)[0]
    fs2 = scenedefs.moving_quad_room(7.0 * step, second_offset=0.65)[0]
    assert len(fs1.arrays["matrices"]) == len(fs0.arrays["matrices"]) + 2 == len(fs2.arrays["matrices"])
    r = new_context(fs0, cam, w, h, fif=fif)
    try:
        r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=2)
        r.updateBVH(fs1)
        r.svgf_render(w, h, DEPTH, 3, frame=1, compute_motion=2)
        got, plane = r.svgf_buffer("motion_depth"), r.svgf_buffer("primary_hit")
        ids = unpack_primary_hit(plane)
        assert (ids["objid"] == info["instance"]).sum() > 50 and (ids["objid"] == info["instance"] + 1).sum() > 50
        assert np.all(got[ids["objid"] >= 0][:, :2] == 0)
        now = host_scene(fs1)
        want, _ = twin_of_frame(r, plane, now, now)
        assert np.array_equal(bits(got), bits(want))
        st = r.geometry_motion_stats()
        assert st["copies"] == 1 and st["copied_float4"] == 4 * len(fs1.arrays["matrices"])
        r.updateBVH(fs2)
        r.svgf_render(w, h, DEPTH, 3, frame=2, compute_motion=2)
        got, plane = r.svgf_buffer("motion_depth"), r.svgf_buffer("primary_hit")
        want, _ = twin_of_frame(r, plane, host_scene(fs2), now)
        check_plane("motion_quad_added_instance_fif%d" % fif, got, want)
        ids = unpack_primary_hit(plane)
        first, second = ids["objid"] == info["instance"], ids["objid"] == info["instance"] + 1
        assert np.allclose(got[first][:, 0] * w, -3.0, atol=1e-3) and np.all(got[second][:, 0] < 0) and second.sum() > 50
    finally:
        r.close()


# ---- 4. the history is the previous FRAME's geometry, not the previous tick's ------------------------------------------------------
def test_two_ticks_between_two_frames(skinned):
    w, h = SIZES[0]
    r = new_context(skinned.fs0, skinned.cam, w, h)
    try:
        skin = skinned.create_skin(r)
        skinned.tick(r, skin, 0)
        r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=2)
        hist = skinned.device_scene(r, skin, skinned.ticks[0]["fs"])
        skinned.tick(r, skin, 1)
        after_one = skinned.device_scene(r, skin, skinned.ticks[1]["fs"])
        skinned.tick(r, skin, 2)
        now = skinned.device_scene(r, skin, skinned.ticks[2]["fs"])
        before = r.geometry_motion_stats()
        r.svgf_render(w, h, DEPTH, 3, frame=1, compute_motion=2)
        got, plane = r.svgf_buffer("motion_depth"), r.svgf_buffer("primary_hit")
        want, _ = twin_of_frame(r, plane, now, hist)
        check_plane("motion_skinned_two_ticks", got, want)
        # the skin's own `prev` is the previous tick's: another plane
        prev_tick = dict(now, vtx=now["vtx"].copy())
        sl = slice(skinned.v0, skinned.v0 + len(skinned.sv))
        prev_tick["vtx"][sl, :3] = r.skin_buffer(skin, "prev")[:, :3]
        assert np.array_equal(bits(prev_tick["vtx"][sl, :3]), bits(after_one["vtx"][sl, :3]))
        other, _ = twin_of_frame(r, plane, now, prev_tick)
        assert not np.array_equal(bits(other), bits(want))
        # the two ticks wrote the same ranges: each is copied once
        st = r.geometry_motion_stats()
        n_mtx = 4 * len(skinned.fs0.arrays["matrices"])
        assert st["copies"] - before["copies"] == 2 and st["copied_float4"] - before["copied_float4"] == len(skinned.sv) + n_mtx
    finally:
        r.close()


# ---- 5. what SVGF and ReSTIR make of the plane -----------------------------------------------------------------------------------
def test_planes_fed_to_a_second_context_give_the_same_frames(skinned):
    w, h = SIZES[0]
    a, b = new_context(skinned.fs0, skinned.cam, w, h), new_context(skinned.fs0, skinned.cam, w, h, motion=False)
    try:
        sa, sb = skinned.create_skin(a), skinned.create_skin(b)
        for k in range(3):
            if k:
                skinned.tick(a, sa, k - 1); skinned.tick(b, sb, k - 1)
            oa, sta = a.svgf_render(w, h, DEPTH, 3, frame=k, compute_motion=2, stages=True)
            b.svgf_set_motion_depth(a.svgf_buffer("motion_depth"))
            ob, stb = b.svgf_render(w, h, DEPTH, 3, frame=k, compute_motion=0, stages=True)
            assert np.array_equal(bits(oa), bits(ob)) and np.array_equal(bits(sta), bits(stb)), k
            for name in ("prev_color_variance", "prev_moment_temporalweight"):
                assert np.array_equal(bits(a.svgf_buffer(name)), bits(b.svgf_buffer(name))), (k, name)
            ra = a.restir_render(w, h, DEPTH, 3, frame=k, compute_motion=2)
            b.restir_set_motion_depth(a.restir_buffer("motion"))
            rb = b.restir_render(w, h, DEPTH, 3, frame=k, compute_motion=0)
            assert np.array_equal(bits(ra), bits(rb)), k
    finally:
        a.close(); b.close()


# ---- 6. frames in flight -----------------------------------------------------------------------------------------------------------
def test_three_frames_in_flight_equal_one(skinned):
    """Ticks and frames enqueued back to back (nothing is read in between), then tick by tick with the planes read."""
    w, h = SIZES[0]
    outs = {}
    for fif in (1, 3):
        r = new_context(skinned.fs0, skinned.cam, w, h, fif=fif)
        try:
            skin = skinned.create_skin(r)
            got = []
            for k in range(3):
                skinned.tick(r, skin, k)
                r.svgf_render(w, h, DEPTH, 3, frame=k, compute_motion=2, download=False)
                r.restir_render(w, h, DEPTH, 3, frame=k, compute_motion=2, download=False)
            got += [r.svgf_buffer(n) for n in ("output", "motion_depth", "prev_color_variance", "prev_moment_temporalweight")]
            got += [r.download_film(), r.restir_buffer("motion")]
            for k in (3, 1, 2):
                skinned.tick(r, skin, k)
                got.append(r.svgf_render(w, h, DEPTH, 3, frame=k + 3, compute_motion=2).copy())
                got.append(r.svgf_buffer("motion_depth"))
                got.append(r.restir_render(w, h, DEPTH, 3, frame=k + 3, compute_motion=2).copy())
            outs[fif] = got
        finally:
            r.close()
    assert len(outs[1]) == len(outs[3]) == 15
    for i, (x, y) in enumerate(zip(outs[1], outs[3])):
        assert np.array_equal(bits(x), bits(y)), i
    for i in (1, 7, 10, 13):
        assert np.count_nonzero(outs[1][i][..., :2]) > 0, i


# ---- 7. the newly covered strip ---------------------------------------------------------------------------------------------------
def test_strip_keeps_its_history_with_mode_2_and_loses_it_with_mode_1(quads):
    fs0, fs1, cam, info = quads
    w, h = SIZES[1]
    weights, planes = {}, {}
    for mode in (2, 1):
        r = new_context(fs0, cam, w, h, motion=mode == 2)
        try:
            r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=mode)
            if mode == 2:
                before = unpack_primary_hit(r.svgf_buffer("primary_hit"))["objid"] == info["instance"]
            r.updateBVH(fs1)
            r.svgf_render(w, h, DEPTH, 3, frame=1, compute_motion=mode)
            if mode == 2:
                after = unpack_primary_hit(r.svgf_buffer("primary_hit"))["objid"] == info["instance"]
            weights[mode] = r.svgf_buffer("prev_moment_temporalweight")[..., 3].copy()
            planes[mode] = r.svgf_buffer("motion_depth")
        finally:
            r.close()
    counted = counted_strip(before, after)
    assert counted.any(1).sum() == after.any(1).sum() - 2 * MARGIN_ROWS >= 6
    assert np.allclose(planes[2][after][:, 0] * w, -SHIFT_COLUMNS, atol=1e-3) and np.all(planes[1][..., :2] == 0)
    assert np.all(weights[2][counted] > 0)
    assert np.all(weights[1][counted] == 0)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_tracking_off_changes_nothing(quads):
    fs0, fs1, cam, info = quads
    w, h = SIZES[0]
    plain, r = new_context(fs0, cam, w, h, motion=False), new_context(fs0, cam, w, h, motion=False)
    try:
        assert status_of(lambda: r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=2)) == INVALID_ARG
        assert status_of(lambda: r.restir_render(w, h, DEPTH, 3, frame=0, compute_motion=2)) == INVALID_ARG
        r.set_geometry_motion(True)
        assert status_of(lambda: r.svgf_render(w, h, DEPTH, 3, spp=2, frame=0, compute_motion=2)) == UNSUPPORTED
        r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=2)
        assert status_of(lambda: r.svgf_denoise(w, h, frame=1, compute_motion=2)) == UNSUPPORTED
        r.svgf_render(w, h, DEPTH, 3, frame=1, compute_motion=1)
        assert status_of(lambda: r.svgf_buffer("primary_hit")) == INVALID_ARG            # the last frame captured no ids
        r.set_geometry_motion(False)
        assert status_of(lambda: r.svgf_render(w, h, DEPTH, 3, frame=0, compute_motion=2)) == INVALID_ARG
        # switched off again: films and SVGF frames are those of a context that never heard of it
        r.svgf_reset(); r.reset()
        for frame in range(2):
            if frame:
                plain.updateBVH(fs1); r.updateBVH(fs1)
            assert np.array_equal(bits(plain.render(w, h, DEPTH, 3, frame=frame)), bits(r.render(w, h, DEPTH, 3, frame=frame)))
            assert np.array_equal(bits(plain.svgf_render(w, h, DEPTH, 3, frame=frame, compute_motion=1)),
                                  bits(r.svgf_render(w, h, DEPTH, 3, frame=frame, compute_motion=1)))
        assert r.geometry_motion_stats()["passes"] == 1
        r.scene_device_arrays()
        assert status_of(lambda: r.set_geometry_motion(True)) == UNSUPPORTED
    finally:
        plain.close(); r.close()
