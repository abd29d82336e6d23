"""ctypes binding of tests/cxx/sphere_oracle.cpp, the CPU twin of atn_set_sphere_intersection(1): the oracle's walk plus the sphere leaf's
step, under the oracle's frame loop and HitTestToTargetLight.  TEST INFRASTRUCTURE ONLY: compiled with g++ into a temporary directory
once per session, loaded by tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "sphere_oracle.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="sphere_oracle_")
        so = os.path.join(_dir, "libsphere_oracle.so")
        # (the oracle's own flags, oracle/Makefile: the closure test holds the two frame loops to each other byte for byte)
        subprocess.check_call(["g++", "-O3", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-o", so, SRC])
        _lib = C.CDLL(so)
    return _lib


def trace_closest(scene, rays, t_min=1e-9, t_max=np.finfo(np.float32).max):
    """INTERSECTION [n] of the twin's walk: a sphere leaf's hit has tri_id = -1, a = t, b = 0, mtrlid = sphere.mtrl_id."""
    from aten_amd import layout as L
    rays = np.ascontiguousarray(rays)
    out = np.zeros(len(rays), L.INTERSECTION)
    lib().sorc_trace_closest(scene.ref(), C.c_void_p(rays.ctypes.data), C.c_uint32(len(rays)), C.c_float(t_min), C.c_float(t_max),
                             C.c_void_p(out.ctypes.data))
    return out


def shadow_visible(scene, queries):
    """HitTestToTargetLight per query (orc.shadow_queries) over the twin's walk: uint8 [n]."""
    from aten_amd import layout as L
    q = np.ascontiguousarray(queries, L.SHADOW_QUERY)
    vis = np.zeros(len(q), np.uint8)
    lib().sorc_shadow_visible(scene.ref(), C.c_void_p(q.ctypes.data), C.c_uint32(len(q)), C.c_void_p(vis.ctypes.data))
    return vis


def render(scene, cam, seeds, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, film=None, progressive=True, nthreads=0):
    """orc.render over the twin's walk: film [h, w, 4]."""
    if film is None:
        film = np.zeros((height, width, 4), np.float32)
    d = orc.Destination(width, height, max_depth, rr_depth, spp, frame, 1 if progressive else 0, nthreads)
    lib().sorc_render(scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), C.c_uint32(len(seeds)),
                      C.byref(d), C.c_void_p(film.ctypes.data), None)
    return film
