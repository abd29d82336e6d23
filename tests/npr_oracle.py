"""ctypes binding of tests/cxx/npr_oracle.cpp, the CPU restatement of the reference's NPR path tracer with feature lines.  TEST
INFRASTRUCTURE ONLY: compiled with g++ into a temporary directory once per session, loaded by tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "npr_oracle.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="npr_oracle_")
        so = os.path.join(_dir, "libnpr_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-o", so, SRC])
        l = C.CDLL(so)
        vp, f, i = C.c_void_p, C.c_float, C.c_int32
        l.orc_npr_create.restype = vp
        l.orc_npr_destroy.argtypes = [vp]
        l.orc_npr_reset.argtypes = [vp]
        l.orc_npr_render.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, i, i, vp, vp, vp, vp, vp, vp]
        l.orc_npr_render.restype = C.c_int
        l.orc_npr_pixel_width.argtypes = [vp, f]; l.orc_npr_pixel_width.restype = f
        l.orc_npr_generate_disc.argtypes = [vp, vp, f, f, vp]
        l.orc_npr_disc_position.argtypes = [f, f, vp, vp]
        l.orc_npr_disc_at.argtypes = [vp, vp, f, f, f, vp]
        l.orc_npr_plane_hit.argtypes = [vp, vp, vp, vp, vp]; l.orc_npr_plane_hit.restype = i
        l.orc_npr_project.argtypes = [vp, vp, vp, vp]; l.orc_npr_project.restype = f
        l.orc_npr_next_ray.argtypes = [f, f, vp, vp, vp, vp, vp]; l.orc_npr_next_ray.restype = i
        l.orc_npr_depth_threshold.argtypes = [vp, f, vp, vp, vp, vp, f, f]; l.orc_npr_depth_threshold.restype = f
        l.orc_npr_in_line_width.argtypes = [f, vp, vp, vp, f, f]; l.orc_npr_in_line_width.restype = i
        l.orc_npr_metrics.argtypes = [vp, vp, vp, i, vp, vp, i, vp, vp, f, f, i, f, f]; l.orc_npr_metrics.restype = i
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _f(v, n=None):
    a = np.ascontiguousarray(v, np.float32)
    assert n is None or a.size == n
    return a


# ---- geometry (feature_line.h), for hand-worked cases
def pixel_width(cam, d=1.0):
    return float(lib().orc_npr_pixel_width(C.c_void_p(cam.ctypes.data), d))


def generate_disc(org, dir, line_width, pixel_width):
    """-> float32[8] {center.xyz, radius, normal.xyz, accumulated_distance}"""
    out = np.zeros(8, np.float32)
    o, d = _f(org, 3), _f(dir, 3)
    lib().orc_npr_generate_disc(_p(o), _p(d), line_width, pixel_width, _p(out))
    return out


def disc_position(u, v, disc):
    out = np.zeros(3, np.float32)
    dd = _f(disc, 8)
    lib().orc_npr_disc_position(u, v, _p(dd), _p(out))
    return out


def disc_at(p, dir, prev_radius, cur, acc_without):
    out = np.zeros(8, np.float32)
    a, b = _f(p, 3), _f(dir, 3)
    lib().orc_npr_disc_at(_p(a), _p(b), prev_radius, cur, acc_without, _p(out))
    return out


def plane_hit(n, p, org, dir):
    out = np.zeros(3, np.float32)
    a, b, c, d = _f(n, 3), _f(p, 3), _f(org, 3), _f(dir, 3)
    return bool(lib().orc_npr_plane_hit(_p(a), _p(b), _p(c), _p(d), _p(out))), out


def project(point, org, dir):
    """-> (distance from the ray, projected point, its distance from the ray origin)"""
    out = np.zeros(4, np.float32)
    a, b, c = _f(point, 3), _f(org, 3), _f(dir, 3)
    d = float(lib().orc_npr_project(_p(a), _p(b), _p(c), _p(out)))
    return d, out[:3].copy(), float(out[3])


def next_ray(u, v, prev_pos, prev_nml, prev_disc, next_disc):
    """-> None (the ray is dropped) or (org, dir)"""
    out = np.zeros(6, np.float32)
    a, b, c, d = _f(prev_pos, 3), _f(prev_nml, 3), _f(prev_disc, 8), _f(next_disc, 8)
    if not lib().orc_npr_next_ray(u, v, _p(a), _p(b), _p(c), _p(d), _p(out)):
        return None
    return out[:3].copy(), out[3:].copy()


def depth_threshold(p, scale, pq, nq, ps, ns, dq, ds):
    a, b, c, d, e = _f(p, 3), _f(pq, 3), _f(nq, 3), _f(ps, 3), _f(ns, 3)
    return float(lib().orc_npr_depth_threshold(_p(a), scale, _p(b), _p(c), _p(d), _p(e), dq, ds))


def in_line_width(w, org, dir, point, acc, pixel_width):
    a, b, c = _f(org, 3), _f(dir, 3), _f(point, 3)
    return bool(lib().orc_npr_in_line_width(w, _p(a), _p(b), _p(c), acc, pixel_width))


def metrics(p, q, s, aq, as_, albedo_threshold, normal_threshold, flags, dq, ds):
    """q / s: (pos, normal, mesh id)."""
    arrs = [_f(p, 3), _f(q[0], 3), _f(q[1], 3), _f(s[0], 3), _f(s[1], 3), _f(aq, 4), _f(as_, 4)]
    return bool(lib().orc_npr_metrics(_p(arrs[0]), _p(arrs[1]), _p(arrs[2]), int(q[2]), _p(arrs[3]), _p(arrs[4]), int(s[2]),
                                      _p(arrs[5]), _p(arrs[6]), albedo_threshold, normal_threshold, flags, dq, ds))


class NPR:
    """Frame-persistent NPR state on the CPU (the per-pixel SampleRayInfo, and contributes_ of the two-pass mode)."""

    def __init__(self):
        self._h = C.c_void_p(lib().orc_npr_create())
        self.film = None

    def close(self):
        if self._h:
            lib().orc_npr_destroy(self._h)
            self._h = None

    def reset(self):
        lib().orc_npr_reset(self._h)
        self.film = None

    def render(self, scene, cam, seeds, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, progressive=True,
               break_on_terminate=True, two_pass=False, nthreads=0, stages=False):
        """One frame into self.film.  Returns the film, and with stages=True a dict: line (found, bounce, distance), desc (u, v, live
        [h, w, 8]), terminated (the path ended at bounce 0), disc (center, radius, normal, acc),
        dims, prim (hit, mesh, depth, albedo_lum, normal) of the primary hit."""
        if self.film is None or self.film.shape[:2] != (height, width):
            self.film = np.zeros((height, width, 4), np.float32)
        n = width * height
        line = np.zeros((height, width, 4), np.float32) if stages else None
        desc = np.zeros((height, width, 8, 4), np.float32) if stages else None
        disc = np.zeros((height, width, 2, 4), np.float32) if stages else None
        dims = np.zeros((height, width), np.uint32) if stages else None
        prim = np.zeros((height, width, 2, 4), np.float32) if stages else None
        d = orc.Destination(width, height, max_depth, rr_depth, spp, frame, 1 if progressive else 0, nthreads)
        lib().orc_npr_render(self._h, scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), len(seeds), C.byref(d),
                             int(break_on_terminate), int(two_pass), _p(self.film), _p(line), _p(desc), _p(disc), _p(dims), _p(prim))
        if not stages:
            return self.film.copy()
        st = dict(line=dict(found=line[..., 0] != 0, bounce=line[..., 1].astype(np.int32), distance=line[..., 2].copy()),
                  desc=dict(u=desc[..., 0].copy(), v=desc[..., 1].copy(), live=desc[..., 2] != 0),
                  terminated=desc[..., 0, 3] != 0,
                  disc=dict(center=disc[..., 0, :3].copy(), radius=disc[..., 0, 3].copy(), normal=disc[..., 1, :3].copy(),
                            acc=disc[..., 1, 3].copy()),
                  dims=dims,
                  prim=dict(hit=prim[..., 0, 0] != 0, mesh=prim[..., 0, 1].astype(np.int32), depth=prim[..., 0, 2].copy(),
                            albedo_lum=prim[..., 0, 3].copy(), normal=prim[..., 1, :3].copy()))
        return self.film.copy(), st
