"""Scenes of the top-layer rebuild tests (tests/test_tlas_oracle_cpu.py clears them, tests/test_gpu_tlas.py renders them).
TEST INFRASTRUCTURE ONLY."""
import numpy as np

from aten_amd import layout as L

W, H = 160, 120
SIZES = [1, 2, 3, 7, 64, 65, 1024, 1025, 4097]


def rigid(rng, spread):
    """A rotation about a random axis and a translation inside a cube of edge `spread`, float32 [4, 4]."""
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    a = rng.uniform(-np.pi, np.pi)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    M[:3, 3] = rng.uniform(-0.5 * spread, 0.5 * spread, 3)
    return M.astype(np.float32)


def set_matrix(fs, inst, M):
    """Instance `inst` of fs gets the L2W matrix M (and its inverse), in place."""
    mid = int(fs.arrays["objects"][inst]["mtx_id"])
    fs.arrays["matrices"][mid] = np.asarray(M, np.float32)
    fs.arrays["matrices"][mid + 1] = np.linalg.inv(np.asarray(M, np.float64)).astype(np.float32)


def quad_instances(n, seed=0):
    """n instances of one two-triangle quad mesh: random rigid matrices, and (from three instances on) one instance without a
    matrix (mtx_id = -1) and one whose matrices are exactly the identity.  Returns (FlatScene, instance object ids)."""
    from aten_amd.scene.builder import SceneBuilder
    rng = np.random.default_rng(1000 + seed + n)
    b = SceneBuilder()
    m = b.add_material("quad", L.MTRL_DIFFUSE, (0.6, 0.6, 0.6))
    pos = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0]], np.float32)
    oid = b.add_mesh("quad", pos, np.array([[0, 1, 2], [0, 2, 3]], np.int64), m, normals=np.tile(np.float32([0, 0, 1]), (4, 1)))
    spread = 4.0 * max(1.0, n ** (1.0 / 3.0))
    inst = [b.create_instance(oid, None if (n >= 3 and k in (1, 2)) else rigid(rng, spread)) for k in range(n)]
    b.set_background((0.1, 0.1, 0.1))
    fs = b.build()
    if n >= 3:
        fs.arrays["objects"][inst[1]]["mtx_id"] = -1       # (its matrices were the identity: the host-built layer's box is the same)
    return fs, inst


def new_matrices(fs, inst, seed):
    """Every instance that has a matrix (but the identity one) moves: arrays['matrices'] of a tick, float32 [m, 4, 4]."""
    rng = np.random.default_rng(seed)
    n = len(inst)
    spread = 4.0 * max(1.0, n ** (1.0 / 3.0))
    mtx = fs.arrays["matrices"].copy()
    for k, i in enumerate(inst):
        mid = int(fs.arrays["objects"][i]["mtx_id"])
        if mid < 0 or (n >= 3 and k == 2):
            continue
        M = rigid(rng, spread)
        mtx[mid] = M
        mtx[mid + 1] = np.linalg.inv(M.astype(np.float64)).astype(np.float32)
    return mtx


def degenerate_instances(kind, n=300):
    """(objects, matrices, table, boxes) of n instances: kind "identical" -- every box the same; "planar" -- every centre in the
    plane z = 3 (a flat axis of the union of the centres; the boxes themselves are flat in z too)."""
    rng = np.random.default_rng(7)
    objs = np.zeros(n + 1, L.OBJECT_PARAM)
    objs["object_id"] = -1; objs["mtx_id"] = -1; objs["triangle_id"] = -1; objs["light_id"] = -1
    mtx = np.tile(np.eye(4, dtype=np.float32), (2 * n, 1, 1))
    table = np.zeros((n, 4), np.float32)
    for k in range(n):
        objs[k + 1]["type"] = L.OBJ_INSTANCE; objs[k + 1]["object_id"] = 0; objs[k + 1]["mtx_id"] = 2 * k
        t = (1.0, 2.0, 3.0) if kind == "identical" else (rng.uniform(-9, 9), rng.uniform(-9, 9), 3.0)
        mtx[2 * k, :3, 3] = t
        mtx[2 * k + 1, :3, 3] = -np.float32(t)
        table[k] = (k + 1, -1.0, np.uint32(1).view(np.float32), 0.0)
    boxes = np.tile(np.float32([-0.5, -0.5, 0, 0.5, 0.5, 0]), (n, 1))
    return objs, mtx, table, boxes


# ---- the rendered scenes: (name, tick) -> FlatScene as the host builds it (objects, matrices, SAH top layer) -------------------------
def cornell_ticks():
    """cornell_box_variant with its two boxes moving: three ticks.  Every tick has the same bottom-level lists."""
    from aten_amd.scene import scenedefs
    out = []
    cam = None
    for k in range(4):          # [0] is the uploaded scene
        fs, cam = scenedefs.cornell_box_variant()
        a = fs.arrays
        # the two instances with a non-identity matrix are the boxes (tall first: scenedefs.cornell_box_variant)
        moved = [i for i, o in enumerate(a["objects"]) if o["type"] == L.OBJ_INSTANCE and o["mtx_id"] >= 0
                 and not np.array_equal(a["matrices"][o["mtx_id"]], np.eye(4, dtype=np.float32))]
        assert len(moved) == 2
        if k:
            for j, i in enumerate(moved):
                ang = np.radians((17.0, -23.0)[j] + 11.0 * k * (1 - 2 * j))
                c, s = np.cos(ang), np.sin(ang)
                t = ((0.15 - 0.05 * k, 0.0, 0.1 + 0.04 * k), (-0.2 + 0.06 * k, 0.25 + 0.05 * k, 0.05))[j]
                set_matrix(fs, i, np.array([[c, 0, s, t[0]], [0, 1, 0, t[1]], [-s, 0, c, t[2]], [0, 0, 0, 1]], np.float32))
            rebuild_host_top(fs)
        out.append(fs)
    return out, cam


def quad_room_ticks():
    """moving_quad_room with the quad (and a second instance of it) at four offsets: [0] is the uploaded scene."""
    from aten_amd.scene import scenedefs
    out, cam = [], None
    for off in (0.0, 0.13, 0.31, -0.17):
        fs, cam, _ = scenedefs.moving_quad_room(off, second_offset=0.4 - off)
        out.append(fs)
    return out, cam


def rebuild_host_top(fs):
    """fs gets a top layer built by the host builder over its CURRENT objects and matrices (after set_matrix) -- what a caller of
    updateBVH hands over -- as SceneBuilder.build does it: the lists' root boxes through the L2W matrices, atns_build_tlas."""
    import ctypes as C
    from aten_amd._hostlib import hostlib
    a = fs.arrays
    boxes, oids, exids = [], [], []
    for oid, o in enumerate(a["objects"]):
        if o["type"] != L.OBJ_INSTANCE:
            continue
        ex = fs.blas_index[int(o["object_id"])]
        root = a["bvh_lists"][ex][0]
        bmin, bmax = root["boxmin"], root["boxmax"]
        corners = np.array([[x, y, z, 1.0] for x in (bmin[0], bmax[0]) for y in (bmin[1], bmax[1]) for z in (bmin[2], bmax[2])], np.float32)
        w = (corners @ a["matrices"][int(o["mtx_id"])].T)[:, :3] if o["mtx_id"] >= 0 else corners[:, :3]
        boxes.append(np.concatenate([w.min(0), w.max(0)])); oids.append(oid); exids.append(ex)
    boxes = np.asarray(boxes, np.float32); oids = np.asarray(oids, np.int32); exids = np.asarray(exids, np.int32)
    mesh_ids = np.full(len(oids), -1, np.int32)
    out = C.c_void_p(); cnt = C.c_uint32()
    lib = hostlib()
    rc = lib.atns_build_tlas(L.ptr(boxes), L.ptr(oids), L.ptr(exids), L.ptr(mesh_ids), len(oids), C.byref(out), C.byref(cnt))
    assert rc == 0
    tlas = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(cnt.value * 48,)).view(L.BVH_NODE).copy()
    lib.atns_free(out)
    fs.replace_bvh_list(0, tlas)
    return fs
