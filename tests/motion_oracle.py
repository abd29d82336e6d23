"""ctypes binding of tests/cxx/motion_oracle.cpp, the CPU twin of the geometry motion pass (docs/MOTION.md).  TEST INFRASTRUCTURE
ONLY: compiled with g++ into a temporary directory once per session, loaded by tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from aten_amd import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "motion_oracle.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="motion_oracle_")
        so = os.path.join(_dir, "libmotion_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so, SRC])
        l = C.CDLL(so)
        vp = C.c_void_p
        l.orc_motion_geometry.argtypes = [vp, C.c_uint32, vp, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        l.orc_motion_geometry.restype = None
        l.orc_motion_static.argtypes = [vp, C.c_uint32, vp, vp, vp]
        l.orc_motion_static.restype = None
        l.orc_motion_sizeof_object.restype = C.c_uint32
        _lib = l
    return _lib


def pack_ids(objid, tri, a, b):
    """The ids plane [..., 4] float32 from int32 object / triangle ids (objid -1 = miss) and the barycentrics."""
    objid = np.asarray(objid, np.int32)
    out = np.zeros(objid.shape + (4,), np.float32)
    out[..., 0] = objid.view(np.float32)
    out[..., 1] = np.asarray(tri, np.int32).view(np.float32)
    out[..., 2] = a
    out[..., 3] = b
    return out


def world_to_clip(pos, at, vfov, aspect, up=(0.0, 1.0, 0.0), znear=0.1, zfar=10000.0):
    """A world-to-clip matrix float32 [4, 4] of the renderer's form (mat4::perspective * mat4::lookat), computed in float64 and
    rounded: for tests that need A camera, not the renderer's own bits (those come from geometry_motion_matrices)."""
    e, c, u = (np.asarray(v, np.float64) for v in (pos, at, up))
    z = e - c; z /= np.linalg.norm(z)
    x = np.cross(u, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    w2v = np.eye(4)
    w2v[0, :3], w2v[1, :3], w2v[2, :3] = x, y, z
    w2v[:3, 3] = -x @ e, -y @ e, -z @ e
    fh = 1.0 / np.tan(np.radians(vfov) * 0.5)
    v2c = np.zeros((4, 4))
    v2c[0, 0], v2c[1, 1] = fh / aspect, fh
    v2c[2, 2], v2c[2, 3] = zfar / (znear - zfar), znear * zfar / (znear - zfar)
    v2c[3, 2] = -1.0
    return (v2c @ w2v).astype(np.float32)


# ---- the moved-quad case shared by the CPU and the GPU tests (scenedefs.moving_quad_room) ----
SHIFT_COLUMNS = 6           # s: the quad moves by this many pixel columns between the two frames (s >= 4)
MARGIN_COLUMNS, MARGIN_ROWS = 2, 2


def column_width(cam, w, h, z):
    """World width of one pixel column in the plane z = const in front of the room's camera (it looks down -z)."""
    dist = cam["pos"][2] - z
    return 2.0 * dist * np.tan(np.radians(cam["vfov"]) * 0.5) * (w / h) / w


def quad_rooms(w=96, h=64, s=SHIFT_COLUMNS):
    """(scene before, scene after, camera, info): the quad moved by s pixel columns along camera-right."""
    from aten_amd.scene import scenedefs
    fs0, cam, info = scenedefs.moving_quad_room(0.0)
    off = s * column_width(cam, w, h, scenedefs.MOVING_QUAD["centre"][2])
    fs1, _, info1 = scenedefs.moving_quad_room(off)
    assert info == info1
    return fs0, fs1, cam, info


def ids_of(isects, w, h):
    """The ids plane [h, w, 4] of a frame's closest hits (layout.INTERSECTION in pixel order)."""
    hit = isects["objid"] >= 0
    return pack_ids(np.where(hit, isects["objid"], -1), np.where(hit, isects["tri_id"], -1), np.where(hit, isects["a"], 0.0),
                      np.where(hit, isects["b"], 0.0)).reshape(h, w, 4)


def counted_strip(quad_before, quad_after):
    """Pixels of the strip the quad newly covers, at least MARGIN_COLUMNS inside both strip edges and MARGIN_ROWS inside the quad."""
    strip = quad_after & ~quad_before
    rows = quad_after.any(1) & quad_before.any(1)
    ys = np.nonzero(rows)[0]
    out = np.zeros_like(strip)
    for y in ys[MARGIN_ROWS:len(ys) - MARGIN_ROWS]:
        xs = np.nonzero(strip[y])[0]
        if len(xs) and xs[-1] - xs[0] + 1 == len(xs):
            out[y, xs[MARGIN_COLUMNS:len(xs) - MARGIN_COLUMNS]] = True
    return out


def motion_geometry(ids, objects, triangles, cur_vtx, h_vtx, cur_mtx, h_mtx, w2c, prev_w2c):
    """The twin: (motion plane, current world positions), shaped like `ids`.  objects: layout.OBJECT_PARAM; triangles:
    layout.TRIANGLE_PARAM; vertices float32 [V, 4]; matrices float32 [M, 4, 4] (M may be 0)."""
    ids = np.ascontiguousarray(ids, np.float32)
    n = ids.size // 4
    objects = np.ascontiguousarray(objects)
    assert objects.dtype.itemsize == lib().orc_motion_sizeof_object()
    tr = np.ascontiguousarray(triangles, L.TRIANGLE_PARAM)
    cv, hv = (np.ascontiguousarray(v, np.float32).reshape(-1, 4) for v in (cur_vtx, h_vtx))
    cm, hm = (np.ascontiguousarray(m, np.float32).reshape(-1, 4, 4) for m in (cur_mtx, h_mtx))
    oid = ids.reshape(-1, 4)[:, 0].copy().view(np.int32)
    tid = ids.reshape(-1, 4)[:, 1].copy().view(np.int32)
    hit = oid >= 0
    assert oid[hit].max(initial=-1) < len(objects) and tid[hit].min(initial=0) >= 0 and tid[hit].max(initial=-1) < len(tr)
    used = tr["idx"][tid[hit]]
    assert used.size == 0 or (used.min() >= 0 and used.max() < min(len(cv), len(hv)))
    o = objects[oid[hit]]
    mids = o["mtx_id"][o["type"] == L.OBJ_INSTANCE]
    assert mids.size == 0 or mids.max() < min(len(cm), len(hm))
    a, b = (np.ascontiguousarray(m, np.float32).reshape(4, 4) for m in (w2c, prev_w2c))
    out = np.zeros_like(ids)
    pos = np.zeros_like(ids)
    p = lambda x: C.c_void_p(x.ctypes.data)
    lib().orc_motion_geometry(p(ids), n, p(objects), int(L.OBJ_INSTANCE), p(tr), p(cv), p(hv), p(cm) if len(cm) else None,
                              p(hm) if len(hm) else None, p(a), p(b), p(out), p(pos))
    return out, pos


def motion_static(pos, w2c, prev_w2c):
    """motion_depth over a plane of world positions (w = 0: miss)."""
    pos = np.ascontiguousarray(pos, np.float32)
    a, b = (np.ascontiguousarray(m, np.float32).reshape(4, 4) for m in (w2c, prev_w2c))
    out = np.zeros_like(pos)
    p = lambda x: C.c_void_p(x.ctypes.data)
    lib().orc_motion_static(p(pos), pos.size // 4, p(a), p(b), p(out))
    return out
