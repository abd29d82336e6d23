"""Skinning on the device (atn_skin_*, csrc/device/skinning.hpp) against its CPU twin (tests/cxx/skinning_oracle.cpp), bit for bit,
and the deformation tick built on it against the tick that skins on the host: films byte for byte."""
import re

import numpy as np
import pytest

import skinning_oracle as S
from aten_amd import layout as L
from aten_amd.scene.camera import create_camera

pytestmark = pytest.mark.gpu

N_BONES = 8
INVALID_ARG, UNSUPPORTED = -1, -5


def mesh_ranges(fs, oid):
    o = fs.arrays["objects"][oid]
    t0, n = int(o["triangle_id"]), int(o["triangle_num"])
    tr = fs.arrays["triangles"][t0:t0 + n]
    v0, v1 = int(tr["idx"].min()), int(tr["idx"].max()) + 1
    return dict(list=fs.blas_index[oid], t0=t0, n=n, v0=v0, v1=v1)


class Room:
    """skinned_room and its first three ticks as the host computes them: the twin's vertices, areas and box, and the scene rebuilt
    around them for the top layer (the caller's business on both paths)."""

    def __init__(self, nu, nv, n_ticks=3):
        from aten_amd.scene import scenedefs
        self.b, self.oid, self.cam, self.sv = scenedefs.skinned_room(nu, nv, N_BONES)
        self.fs0 = self.b.build()
        self.d = mesh_ranges(self.fs0, self.oid)
        d = self.d
        assert d["v1"] - d["v0"] == len(self.sv) == 3 * d["n"]
        assert len(self.fs0.arrays["bvh_lists"][d["list"]]) == 2 * d["n"] - 1          # one triangle per leaf
        twin = S.SkinTwin(self.sv, self.fs0.arrays["triangles"][d["t0"]:d["t0"] + d["n"]], vtx_offset=d["v0"])
        self.ticks = []
        for k in range(n_ticks):
            pal = scenedefs.skinned_pose(0.9 * k + 0.4, N_BONES)
            twin.compute(pal, k == 0)
            self.b.set_mesh_vertices(self.oid, twin.pos[:, :3], np.arange(len(self.sv)).reshape(-1, 3), twin.nml[:, :3])
            fs = self.b.build()
            assert mesh_ranges(fs, self.oid) == d
            self.ticks.append(dict(palette=pal, restart=k == 0, pos=twin.pos.copy(), nml=twin.nml.copy(), prev=twin.prev.copy(),
                                   tris=twin.tris.copy(), bbox=twin.bbox.copy(), fs=fs))


@pytest.fixture(scope="module")
def room():
    return Room(48, 24)


def new_context(fs, cam, W, H, fif=1, twins=None, planar=None):
    from aten_amd.renderer import PathTracing
    r = PathTracing(0)
    try:
        if twins is not None or planar is not None:
            r.set_upload_options(anyhit_twin=None if twins is None else (2 if twins else 0), planar_lights=planar)
        r.UpdateSceneData(fs)
        r.updateCamera(create_camera(cam["pos"], cam["at"], cam["vfov"], W, H))
        r.initSampler(W, H, 0)
        r.set_frames_in_flight(fif)
    except Exception:
        r.close()
        raise
    return r


def run_ticks(room, mode, W, H, fif, twins):
    """Three ticks with frames of the previous geometry in flight in front of each; the film after every tick, the counters of
    a counted frame at the end, and the rebuilt list's bytes.  mode: "host" (the twin's vertices through updateGeometry),
    "device" (skin_compute returning the box) or "device_noreadback" (the box never leaves the device)."""
    d = room.d
    r = new_context(room.fs0, room.cam, W, H, fif, twins)
    try:
        assert (r.anyhit_twins() >= 1) if twins else (r.anyhit_twins() == 0)
        skin = None if mode == "host" else r.skin_create(room.sv, d["v0"], d["t0"], d["n"], N_BONES)
        films, boxes, lists = [], [], []
        for k, t in enumerate(room.ticks):
            for f in range(fif):
                r.render(W, H, frame=f, download=False)
            if mode == "host":
                r.updateGeometry(vtx_pos=t["pos"], vtx_nml=t["nml"], vtx_offset=d["v0"], triangles=t["tris"], tri_offset=d["t0"])
                r.lbvh_rebuild_list(d["list"], d["t0"], d["n"], t["bbox"][:3], t["bbox"][3:])
            elif mode == "device":
                r.skin_update(skin, t["palette"])
                mn, mx = r.skin_compute(skin, t["restart"])
                boxes.append(np.concatenate([mn, mx]))
                r.lbvh_rebuild_list(d["list"], d["t0"], d["n"], mn, mx)
            else:
                r.skin_update(skin, t["palette"])
                assert r.skin_compute(skin, t["restart"], want_bbox=False) is None
                r.lbvh_rebuild_list_skinned(d["list"], skin)
            r.updateBVH(t["fs"])
            r.reset()
            films.append(r.render(W, H, frame=7 + k).copy())
            lists.append(r.bvh_list_bytes(d["list"]).copy())
        r.set_frames_in_flight(1)
        r.reset()
        films.append(r.render(W, H, frame=11, count_stats=True).copy())
        return dict(films=films, stats=r.stats(), boxes=boxes, lists=lists)
    finally:
        r.close()


# ---- 1. bit parity with the twin ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_room_context():
    """A room whose tube has 100 800 vertices (33 600 triangles): skins of every size are bound to its leading vertices."""
    from aten_amd.scene import scenedefs
    b, oid, cam, sv = scenedefs.skinned_room(160, 105, 4)
    fs = b.build()
    r = new_context(fs, cam, 64, 64)
    yield r, fs, mesh_ranges(fs, oid)
    r.close()


@pytest.mark.parametrize("n_matrices", [1, 4, 200])
@pytest.mark.parametrize("n_vertices", [1, 63, 64, 65, 257, 4099, 100003])
def test_skinning_equals_the_twin_bit_for_bit(big_room_context, n_vertices, n_matrices):
    check_against_twin(big_room_context, n_vertices, n_matrices)


@pytest.mark.parametrize("n_vertices", [65, 4099])
def test_skinning_with_the_palette_in_global_memory_equals_the_twin(big_room_context, n_vertices):
    """More than 256 matrices: the flavour of the vertex pass that reads the palette from global memory instead of LDS."""
    check_against_twin(big_room_context, n_vertices, 300)


def check_against_twin(big_room_context, n_vertices, n_matrices):
    r, fs, d = big_room_context
    assert n_vertices <= d["v1"] - d["v0"]
    n_tri = n_vertices // 3                         # the builder stores three vertices per triangle: these lie inside the range
    v = S.random_vertices(n_vertices, n_matrices, 1000 * n_matrices + n_vertices % 997)
    tris = fs.arrays["triangles"][d["t0"]:d["t0"] + n_tri]
    twin = S.SkinTwin(v, tris, vtx_offset=d["v0"])
    skin = r.skin_create(v, d["v0"], d["t0"], n_tri, n_matrices)
    try:
        for k in range(4):
            pal = S.random_palette(n_matrices, 77 * k + n_matrices)
            twin.compute(pal, k == 0)
            r.skin_update(skin, pal)
            mn, mx = r.skin_compute(skin, k == 0)
            got = {name: r.skin_buffer(skin, name) for name in ("pos", "nml", "prev", "bbox", "area")}
            for name, want in (("pos", twin.pos), ("nml", twin.nml), ("prev", twin.prev), ("area", twin.area)):
                assert got[name].shape == want.shape
                assert got[name].tobytes() == want.tobytes(), "%s differs at tick %d: %d of %d values" % (
                    name, k, int((got[name].view(np.uint32) != want.view(np.uint32)).sum()), want.size)
            assert np.array_equal(got["bbox"], twin.bbox)                       # by value
            assert np.array_equal(np.concatenate([mn, mx]), twin.bbox)
    finally:
        r.skin_close(skin)


# ---- 2. / 3. the tick: device against host, with and without the read-back ------------------------------------------------------
@pytest.mark.parametrize("twins", [True, False])
@pytest.mark.parametrize("fif", [1, 3])
@pytest.mark.parametrize("size", [(96, 96), (1920, 1080)])
def test_device_ticks_render_the_host_ticks_films(room, size, fif, twins):
    W, H = size
    host = run_ticks(room, "host", W, H, fif, twins)
    dev = run_ticks(room, "device", W, H, fif, twins)
    for k, t in enumerate(room.ticks):
        assert np.array_equal(dev["boxes"][k], t["bbox"])
    for k, (x, y) in enumerate(zip(host["films"], dev["films"])):
        assert np.isfinite(x[..., :3]).all() and x[..., :3].max() > 0
        assert x.tobytes() == y.tobytes(), "film %d differs in %d pixels" % (k, int((x != y).any(-1).sum()))
    assert host["films"][0].tobytes() != host["films"][1].tobytes()              # the ticks do move the tube
    for k in ("closest_rays", "hits", "closest_nodes", "closest_tris"):
        assert host["stats"][k] == dev["stats"][k], k
    # 3. no read-back: the same films and the same rebuilt list, the box never on the host
    nrb = run_ticks(room, "device_noreadback", W, H, fif, twins)
    for k, (x, y) in enumerate(zip(host["films"], nrb["films"])):
        assert x.tobytes() == y.tobytes(), "film %d differs in %d pixels (no read-back)" % (k, int((x != y).any(-1).sum()))
    for k in ("closest_rays", "hits", "closest_nodes", "closest_tris"):
        assert host["stats"][k] == nrb["stats"][k], k
    for k in range(len(room.ticks)):
        assert len(host["lists"][k]) == len(nrb["lists"][k]) > 0
        assert host["lists"][k].tobytes() == nrb["lists"][k].tobytes() == dev["lists"][k].tobytes(), "list differs at tick %d" % k
    assert host["lists"][0].tobytes() != host["lists"][1].tobytes()


# ---- 4. a tick writes the skin's ranges only ------------------------------------------------------------------------------------
def test_a_tick_touches_only_the_skins_ranges(room):
    d, fs0 = room.d, room.fs0
    nv, nt = len(fs0.arrays["vtx_pos"]), len(fs0.arrays["triangles"])
    W = H = 64
    r = new_context(fs0, room.cam, W, H, fif=3)
    try:
        skin = r.skin_create(room.sv, d["v0"], d["t0"], d["n"], N_BONES)
        before = r.skin_scene_arrays(skin, nv, nt)
        for k in range(4):                          # every copy of the scene a frame in flight may read is written at least once
            t = room.ticks[k % len(room.ticks)]
            for f in range(3):
                r.render(W, H, frame=f, download=False)
            r.skin_update(skin, t["palette"])
            r.skin_compute(skin, k == 0, want_bbox=False)
            r.lbvh_rebuild_list_skinned(d["list"], skin)
            r.updateBVH(t["fs"])
        after = r.skin_scene_arrays(skin, nv, nt)
        t = room.ticks[3 % len(room.ticks)]
        vin = np.zeros(nv, bool); vin[d["v0"]:d["v1"]] = True
        tin = np.zeros(nt, bool); tin[d["t0"]:d["t0"] + d["n"]] = True
        assert (~vin).sum() > 0 and (~tin).sum() > 0
        for name, inside in (("vtx_pos", vin), ("vtx_nml", vin), ("triangles", tin), ("shade", tin)):
            assert after[name][~inside].tobytes() == before[name][~inside].tobytes(), name
            assert after[name][inside].tobytes() != before[name][inside].tobytes(), name
        assert after["vtx_pos"][vin].tobytes() == t["pos"].tobytes() and after["vtx_nml"][vin].tobytes() == t["nml"].tobytes()
        tr = after["triangles"][tin]
        assert tr.tobytes() == t["tris"].tobytes()
        # the skin's shading records: the three positions, the three normals, the triangle's second half, its indices
        sh = after["shade"][tin]
        rel = tr["idx"] - d["v0"]
        for c in range(3):
            assert sh[:, c].tobytes() == t["pos"][rel[:, c]].tobytes() and sh[:, 3 + c].tobytes() == t["nml"][rel[:, c]].tobytes()
        assert sh[:, 6, 0].tobytes() == tr["area"].tobytes()
        assert sh[:, 7, :3].view(np.int32).tobytes() == tr["idx"].tobytes()
    finally:
        r.close()


# ---- 5. the planar-light rule survives ------------------------------------------------------------------------------------------
def test_a_skinning_tick_keeps_the_planar_light_rule(room):
    """As test_gpu_anyhit_twin.test_a_deformation_tick_keeps_the_planar_light_rule: the tick writes the tube, not the lamp, so the
    lamp's shadow rays keep stopping early; frames equal those of a context that never had the rule, with fewer shadow-ray nodes."""
    d = room.d
    W, H = 160, 120
    out = {}
    for rule in (0, 1):
        r = new_context(room.fs0, room.cam, W, H, fif=3, planar=rule)
        try:
            assert r.planar_area_lights() == rule
            skin = r.skin_create(room.sv, d["v0"], d["t0"], d["n"], N_BONES)
            films = []
            for k, t in enumerate(room.ticks[:2]):
                for f in range(3):
                    r.render(W, H, frame=f, download=False)
                r.skin_update(skin, t["palette"])
                r.skin_compute(skin, k == 0, want_bbox=False)
                r.lbvh_rebuild_list_skinned(d["list"], skin)
                r.updateBVH(t["fs"])
                assert r.planar_area_lights() == rule
                r.reset()
                films.append(r.render(W, H, frame=7 + k).copy())
            r.set_frames_in_flight(1)
            r.reset()
            films.append(r.render(W, H, frame=9, count_stats=True).copy())
            out[rule] = (films, r.stats())
        finally:
            r.close()
    for x, y in zip(out[0][0], out[1][0]):
        assert x.tobytes() == y.tobytes()
    s0, s1 = out[0][1], out[1][1]
    for k in ("closest_rays", "shadow_rays", "hits", "closest_nodes", "closest_tris"):
        assert s0[k] == s1[k]
    assert s1["shadow_nodes"] < s0["shadow_nodes"]


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def refused(fn, code):
    from aten_amd.renderer import AtenAmdError
    with pytest.raises(AtenAmdError) as e:
        fn()
    m = re.match(r"^(.+) \(status (-?\d+)\)$", str(e.value), re.S)
    assert m and int(m.group(2)) == code, str(e.value)
    assert len(m.group(1).strip()) > 8, "no message"


def test_refusals_leave_the_context_rendering(room):
    d, fs0, sv = room.d, room.fs0, room.sv
    nv, nt = len(fs0.arrays["vtx_pos"]), len(fs0.arrays["triangles"])
    W = H = 96
    fresh = new_context(fs0, room.cam, W, H)
    try:
        want = fresh.render(W, H, frame=3).copy()
    finally:
        fresh.close()
    r = new_context(fs0, room.cam, W, H)
    try:
        mk = lambda v=sv, v0=d["v0"], t0=d["t0"], n=d["n"], nm=N_BONES: r.skin_create(v, v0, t0, n, nm)
        # ranges outside the scene
        refused(lambda: mk(v0=nv - len(sv) + 1), INVALID_ARG)
        refused(lambda: mk(t0=nt - d["n"] + 1), INVALID_ARG)
        refused(lambda: mk(v=sv[:0]), INVALID_ARG)
        refused(lambda: mk(nm=0), INVALID_ARG)
        # a triangle of the range names a vertex outside the skin's vertices
        refused(lambda: mk(v=sv[3:], v0=d["v0"] + 3), INVALID_ARG)
        refused(lambda: mk(v=sv[:-3]), INVALID_ARG)
        # a blend index outside the palette, also under a weight of 0
        for bad in (float(N_BONES), -1.0, float("nan"), 1e9):
            v = sv.copy()
            v["blend_index"][len(v) // 2, 3] = bad
            v["blend_weight"][len(v) // 2, 3] = 0.0
            refused(lambda: mk(v=v), UNSUPPORTED)
        refused(lambda: mk(nm=N_BONES - 1), UNSUPPORTED)         # the tube's own indices against a shorter palette
        refused(lambda: mk(nm=65537), UNSUPPORTED)
        skin = mk()
        pal = room.ticks[0]["palette"]
        refused(lambda: r.skin_compute(skin, True), INVALID_ARG)                   # before the first update
        refused(lambda: r.lbvh_rebuild_list_skinned(d["list"], skin), INVALID_ARG)  # before the first compute: no box
        refused(lambda: r.skin_update(skin, pal[:-1]), INVALID_ARG)
        refused(lambda: r.skin_update(skin, np.concatenate([pal, pal])), INVALID_ARG)
        r.skin_update(skin, pal)
        mn = np.zeros(3, np.float32)
        assert r._l.atn_skin_compute(r._ctx, skin, 1, mn.ctypes.data, None) == INVALID_ARG and len(r._l.atn_last_error(r._ctx)) > 8
        refused(lambda: r.skin_buffer(skin + 1000, "pos"), INVALID_ARG)
        r.skin_compute(skin, True)
        # the refusals of lbvh_rebuild_list
        refused(lambda: r.lbvh_rebuild_list_skinned(0, skin), INVALID_ARG)
        refused(lambda: r.lbvh_rebuild_list_skinned(len(fs0.arrays["bvh_lists"]), skin), INVALID_ARG)
        other = [i for i in range(1, len(fs0.arrays["bvh_lists"])) if i != d["list"]][0]
        refused(lambda: r.lbvh_rebuild_list_skinned(other, skin), UNSUPPORTED)
        part = r.skin_create(sv[:300], d["v0"], d["t0"], 100, N_BONES)             # a skin over a part of the list's triangles
        r.skin_update(part, pal); r.skin_compute(part, True)
        refused(lambda: r.lbvh_rebuild_list_skinned(d["list"], part), UNSUPPORTED)
        r.skin_close(part)
        # dead handles: destroyed, and older than the last upload
        refused(lambda: r.skin_update(part, pal), INVALID_ARG)
        refused(lambda: r.skin_close(part), INVALID_ARG)
        # atn_update_geometry rewrites one of the skin's triangles with vertices that are not the skin's
        tr = fs0.arrays["triangles"][d["t0"]:d["t0"] + d["n"]].copy()
        tr["idx"][5] = [0, 1, 2]
        r.updateGeometry(triangles=tr, tri_offset=d["t0"])
        refused(lambda: r.skin_compute(skin, False), UNSUPPORTED)
        r.UpdateSceneData(fs0)
        for fn in (lambda: r.skin_update(skin, pal), lambda: r.skin_compute(skin, True), lambda: r.lbvh_rebuild_list_skinned(d["list"], skin),
                   lambda: r.skin_buffer(skin, "pos"), lambda: r.skin_close(skin)):
            refused(fn, INVALID_ARG)
        # the context still renders the uploaded scene
        r.reset()
        assert r.render(W, H, frame=3).tobytes() == want.tobytes()
        # a context whose arrays the caller writes itself
        skin = mk()
        r.skin_update(skin, pal)
        r.scene_device_arrays()
        refused(lambda: r.skin_compute(skin, True), UNSUPPORTED)
        refused(lambda: mk(), UNSUPPORTED)
        r.reset()
        assert r.render(W, H, frame=3).tobytes() == want.tobytes()
    finally:
        r.close()
