"""The trees that tests/test_brute_force_cpu.py and tests/test_gpu_brute_force.py hold to float64 (tests/brute_force.py).
TEST INFRASTRUCTURE ONLY.

A Case names a scene in its FINAL state twice: `host` is that state built by the host builders (what the CPU module walks with the
oracle, and what float64 expands), `upload` + `tick(r)` is how a device context gets there (None: upload `host`).  Nothing here
imports the oracle."""
import numpy as np

import tlas_scenes
from aten_amd import layout as L

NONRIGID = {
    "half": np.diag([0.5, 0.5, 0.5]),
    "double": np.diag([2.0, 2.0, 2.0]),
    "nonuniform": np.diag([1.0, 3.0, 0.25]),
    "shear": np.array([[1.0, 0.6, 0.0], [0.0, 1.0, -0.4], [0.3, 0.0, 1.0]]),
    "mirror": np.diag([1.0, -1.0, 1.0]),
}
LIGHT_POS = {"box7": (0.5, 6.0, 1.0), "half": (0.5, 6.0, 1.0), "sponza": (0.0, 1.5, 0.0)}


class Case:
    def __init__(self, name, host, rule="world", upload=None, tick=None, aim=0.0, rays="sets", clear=False, tris=None, box=1.0, beyond=0.0):
        self.name, self.host, self.rule, self.upload, self.tick = name, host, rule, (host if upload is None else upload), tick
        self.aim, self.rays, self.clear, self.tris, self.box, self.beyond = aim, rays, clear, tris, box, beyond

    def ray_sets(self, tris, seed=1):
        import brute_force as B
        return B.ray_sets(tris, seed, self.rule, aim=self.aim, box=self.box, clear=self.clear)

    def shadow_set(self, tris, light_pos, seed=5):
        import brute_force as B
        return B.shadow_set(tris, light_pos, seed, beyond=self.beyond)


def box_instances(n=7, kind=None, seed=0, light=None):
    """n instances of a 12-triangle box whose local box is OFF-CENTRE (around (3, -2, 5)), each rotated about a random axis and moved;
    kind: a key of NONRIGID, applied before the rotation.  The reference's own aabb::transform (math/aabb.h:307-344) re-adds the box
    centre after the matrix, which is wrong for exactly such a mesh; the product takes the eight corners.  Returns (FlatScene, ids)."""
    from aten_amd.scene.builder import SceneBuilder
    from aten_amd.scene.scenedefs import _box_mesh
    rng = np.random.default_rng(2000 + seed + n)
    b = SceneBuilder()
    m = b.add_material("box", L.MTRL_DIFFUSE, (0.6, 0.6, 0.6))
    p, tri = _box_mesh((2.6, -2.5, 4.7), (3.4, -1.5, 5.3))
    oid = b.add_mesh("box", p, tri, m)
    inst = []
    for k in range(n):
        M = tlas_scenes.rigid(rng, 6.0).astype(np.float64)
        # (the rotation turns about the world origin: the mesh, three to six units from it, swings far; pull it back)
        M[:3, 3] -= M[:3, :3] @ np.array([3.0, -2.0, 5.0])
        if kind is not None:
            K = np.eye(4); K[:3, :3] = NONRIGID[kind]
            c = np.eye(4); c[:3, 3] = (3.0, -2.0, 5.0)
            ci = np.eye(4); ci[:3, 3] = (-3.0, 2.0, -5.0)
            M = M @ c @ K @ ci                           # scaled about the mesh's own centre
        inst.append(b.create_instance(oid, M.astype(np.float32)))
    if light is not None:
        b.add_point_light(light, (1.0, 0.9, 0.8), 20.0)
    b.set_background((0.1, 0.1, 0.1))
    return b.build(), inst


def moved(fs_fresh, inst, seed, kind=None):
    """fs_fresh (a second build of an uploaded scene) with tlas_scenes.new_matrices and a host-built top layer over them."""
    mtx = tlas_scenes.new_matrices(fs_fresh, inst, seed)
    fs_fresh.arrays["matrices"][:] = mtx
    return tlas_scenes.rebuild_host_top(fs_fresh)


def soup_room(kind, n):
    """A floor and a back wall with a deformable mesh that is test_gpu_lbvh.soup(n, n, kind): long runs of equal Morton codes
    ("clustered") and a zero-size axis ("flat").  Returns (FlatScene, rebuild arguments)."""
    from aten_amd.scene.builder import SceneBuilder
    from test_gpu_lbvh import soup
    _, pos = soup(n, n, kind)
    b = SceneBuilder()
    m = b.add_material("grey", L.MTRL_DIFFUSE, (0.6, 0.6, 0.6))
    lo, hi = pos[:, :3].min(0) - 1.0, pos[:, :3].max(0) + 1.0
    floor = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], lo[1], hi[2]], [lo[0], lo[1], hi[2]]], np.float32)
    wall = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]], [lo[0], hi[1], lo[2]]], np.float32)
    b.create_instance(b.add_mesh("floor", floor, [[0, 2, 1], [0, 3, 2]], m))
    b.create_instance(b.add_mesh("wall", wall, [[0, 1, 2], [0, 2, 3]], m))
    oid = b.add_mesh("soup", pos[:, :3], np.arange(3 * n).reshape(n, 3), m, deformable=True)
    b.create_instance(oid)
    b.set_background((0.1, 0.1, 0.1))
    fs = b.build()
    o = fs.arrays["objects"][oid]
    t0 = int(o["triangle_id"])
    assert int(o["triangle_num"]) == n and len(fs.arrays["bvh_lists"][fs.blas_index[oid]]) == 2 * n - 1
    return fs, dict(list=fs.blas_index[oid], t0=t0, n=n, bmin=pos[:, :3].min(0), bmax=pos[:, :3].max(0))


def host_with_lbvh(fs, d, lbvh_build):
    """fs with list d["list"] replaced by lbvh_build's tree (the CPU module passes orc.lbvh_build: the device tree's twin)."""
    tris = fs.arrays["triangles"][d["t0"]:d["t0"] + d["n"]]
    fs.replace_bvh_list(d["list"], lbvh_build(tris, d["bmin"], d["bmax"], fs.arrays["vtx_pos"], tri_id_offset=d["t0"]))
    return fs


def _quads(n, dev):
    fs, inst = tlas_scenes.quad_instances(n)
    if not dev:
        return Case("quad%d" % n, fs, aim=0.4)
    host = moved(tlas_scenes.quad_instances(n)[0], inst, 77 + n)
    mtx = host.arrays["matrices"].copy()
    return Case("quad%d_dev" % n, host, upload=fs, aim=0.4, tick=lambda r: r.tlas_rebuild(matrices=mtx, force_general=(n > 1024)))


def _boxes(kind, dev, light=False):
    name = kind or "box7"
    fs, inst = box_instances(7, kind, light=LIGHT_POS[name] if light else None)
    rule = "world" if kind is None else "local"
    if not dev:
        return Case(name + ("_light" if light else ""), fs, rule, aim=0.4, beyond=0.7)
    host = moved(box_instances(7, None)[0], inst, 91) if kind is None else fs
    mtx = host.arrays["matrices"].copy()
    return Case(name + "_dev", host, rule, upload=fs, aim=0.4, tick=lambda r: r.tlas_rebuild(matrices=mtx))


def _atrium():
    from aten_amd.scene import scenedefs
    fs, cam = scenedefs.atrium(detail=0.25)
    c = Case("atrium", fs, "local", rays="primary")
    c.cam = cam
    return c


def _room_lbvh(t):
    from aten_amd.scene import scenedefs
    from test_gpu_lbvh import tick_data, push_tick
    b, oid, _ = scenedefs.deformable_room(0.0)
    fs0, _ = tick_data(b, oid, 0.0)
    fs, d = tick_data(b, oid, t)
    c = Case("room_lbvh_%g" % t, fs, upload=fs0, tick=lambda r: push_tick(r, fs, d))
    c.lbvh = d          # (the CPU module swaps the oracle's LBVH into `host`)
    return c


def _soup(kind, n):
    fs, d = soup_room(kind, n)
    c = Case("soup_%s" % kind, fs, clear=True, tick=lambda r: r.lbvh_rebuild_list(d["list"], d["t0"], d["n"], d["bmin"], d["bmax"]))
    c.lbvh = d
    return c


_skin_room = []


def skin_room():
    if not _skin_room:
        from test_gpu_skinning import Room
        _skin_room.append(Room(48, 24, n_ticks=2))
    return _skin_room[0]


def _skinned(k):
    """Pose k of test_gpu_skinning's room: skin_update, skin_compute(want_bbox=False), lbvh_rebuild_list_skinned, tlas_rebuild for the
    poses 0 .. k.  `host` is the twin's scene of that pose; a device context expands the vertices it downloads (Case.tris)."""
    from test_gpu_skinning import N_BONES
    room = skin_room()
    d = room.d
    state = {}

    def tick(r):
        skin = r.skin_create(room.sv, d["v0"], d["t0"], d["n"], N_BONES)
        for t in room.ticks[:k + 1]:
            r.skin_update(skin, t["palette"])
            assert r.skin_compute(skin, t["restart"], want_bbox=False) is None
            r.lbvh_rebuild_list_skinned(d["list"], skin)
            r.tlas_rebuild()
        state["skin"] = skin

    def tris(r):
        import brute_force as B
        a = room.fs0.arrays
        dev = r.skin_scene_arrays(state["skin"], len(a["vtx_pos"]), len(a["triangles"]))
        assert np.array_equal(dev["triangles"]["idx"], a["triangles"]["idx"])
        return B.world_triangles(room.fs0, vtx_pos=dev["vtx_pos"])

    c = Case("skinned_%d" % k, room.ticks[k]["fs"], upload=room.fs0, tick=tick, tris=tris)
    c.lbvh = dict(d, bmin=room.ticks[k]["bbox"][:3], bmax=room.ticks[k]["bbox"][3:])
    return c


def _sponza(use_sbvh, light=False):
    from aten_amd.scene import scenedefs
    add = (lambda b, lo, hi, cam: b.add_point_light(LIGHT_POS["sponza"], (1.0, 0.9, 0.8), 20.0)) if light else None
    fs, _ = scenedefs.sponza_lod(use_sbvh=use_sbvh, textures=False, ibl=False, add_lights=add)
    return Case("sponza_%s%s" % ("sbvh" if use_sbvh else "sah", "_light" if light else ""), fs, box=1.6)      # (a closed hall: origins of the inside set also lie around it)


MAKERS = {}
for _n in (3, 65):
    MAKERS["quad%d" % _n] = lambda n=_n: _quads(n, False)
MAKERS["box7"] = lambda: _boxes(None, False)
for _n in (3, 65, 1025):
    MAKERS["quad%d_dev" % _n] = lambda n=_n: _quads(n, True)
MAKERS["box7_dev"] = lambda: _boxes(None, True)
for _k in NONRIGID:
    MAKERS[_k] = lambda k=_k: _boxes(k, False)
    MAKERS[_k + "_dev"] = lambda k=_k: _boxes(k, True)
MAKERS["atrium"] = _atrium
for _t in (0.9, 2.1):
    MAKERS["room_lbvh_%g" % _t] = lambda t=_t: _room_lbvh(t)
MAKERS["soup_clustered"] = lambda: _soup("clustered", 5000)
MAKERS["soup_flat"] = lambda: _soup("flat", 3000)
for _p in (0, 1):
    MAKERS["skinned_%d" % _p] = lambda p=_p: _skinned(p)
MAKERS["sponza_sah"] = lambda: _sponza(False)
MAKERS["sponza_sbvh"] = lambda: _sponza(True)
# Matrices that ENLARGE (|W2L d| < 1 for some d): the reference's walk -- world boxes pruned with a t_max in the instance's smaller unit
# -- gives answers there that depend on its order, neither rule "local" nor "world" (docs/TRACE_GROUND_TRUTH.md).  The product restates
# the reference, so these cases are held to what float64 can assert of ANY order (brute_force.any_order), and the number of decided
# rays off rule "local" is pinned.
ENLARGING = ("double", "nonuniform", "shear")
ANY_ORDER = [n for n in MAKERS if n.split("_")[0] in ENLARGING]
CLOSEST = [n for n in MAKERS if n not in ANY_ORDER]
RIGID = [n for n in CLOSEST if n.split("_")[0] not in NONRIGID and n != "atrium"]
SCALED = [n for n in CLOSEST if n not in RIGID]
SMALL = [n for n in CLOSEST if n.split("_")[0] in ("quad3", "quad65", "box7") + tuple(NONRIGID)]      # node images of at most 32 KiB take the LDS walk: these also run "global"

SHADOW_MAKERS = {
    "box7_light": lambda: _boxes(None, False, light=True),
    "half_light": lambda: _boxes("half", False, light=True),
    "sponza_sbvh_light": lambda: _sponza(True, light=True),
}
SHADOW = list(SHADOW_MAKERS)
_made = {}


def case(name):
    if name not in _made:
        _made[name] = (MAKERS.get(name) or SHADOW_MAKERS[name])()
    return _made[name]


def point_light(fs):
    """(index, position) of the scene's point light."""
    k = int(np.flatnonzero(fs.arrays["lights"]["type"] == L.LIGHT_POINT)[0])
    return k, fs.arrays["lights"][k]["pos"][:3].astype(np.float64)
