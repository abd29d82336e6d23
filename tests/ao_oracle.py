"""ctypes binding of tests/cxx/ao_oracle.cpp, the CPU restatement of the reference's ambient-occlusion renderer.  TEST
INFRASTRUCTURE ONLY: compiled with g++ into a temporary directory once per session, loaded by tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "ao_oracle.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="ao_oracle_")
        so = os.path.join(_dir, "libao_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-o", so, SRC])
        l = C.CDLL(so)
        vp, f, i = C.c_void_p, C.c_float, C.c_int32
        l.orc_ao_create.restype = vp
        l.orc_ao_destroy.argtypes = [vp]
        l.orc_ao_reset.argtypes = [vp]
        l.orc_ao_render.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, i, f, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        l.orc_ao_render.restype = C.c_int
        l.orc_ao_filter.argtypes = [i, i, vp, vp, vp]
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def bilateral(values, depths):
    """RenderAOWithBilateralFilter's two passes and its halving over given planes [h, w] -> the values put into the film."""
    v = np.ascontiguousarray(values, np.float32)
    d = np.ascontiguousarray(depths, np.float32)
    assert v.shape == d.shape and v.ndim == 2
    out = np.zeros_like(v)
    lib().orc_ao_filter(v.shape[1], v.shape[0], _p(v), _p(d), _p(out))
    return out


class AO:
    """Frame-persistent AO state on the CPU (path_host_'s contributions, isects_, the film)."""

    def __init__(self):
        self._h = C.c_void_p(lib().orc_ao_create())
        self.film = None

    def close(self):
        if self._h:
            lib().orc_ao_destroy(self._h)
            self._h = None

    def reset(self):
        lib().orc_ao_reset(self._h)
        self.film = None

    def render(self, scene, cam, seeds, width, height, num_rays=1, radius=1.0, filter=False, frame=0, progressive=True,
               break_on_terminate=True, stale_isect=False, nthreads=0, stages=False):
        """One frame into self.film.  break_on_terminate=True: the CPU renderer as written; False: idaten's miss rule.  Returns the
        film, and with stages=True a dict: state (0 not rendered / 1 hit / 2 miss), value, depth, first_miss [h], ray (org, dir, normal_mapped),
        answer (kind, t, c, skips) of the pixel's first AO ray, answers (the same of all its AO rays [h, w, num_rays]), skips (all AO rays of the pixel)."""
        if self.film is None or self.film.shape[:2] != (height, width):
            self.film = np.zeros((height, width, 4), np.float32)
        state = np.zeros((height, width), np.uint32) if stages else None
        value = np.zeros((height, width), np.float32) if stages else None
        depth = np.zeros((height, width), np.float32) if stages else None
        ray = np.zeros((height, width, 2, 4), np.float32) if stages else None
        ans = np.zeros((height, width, 4), np.float32) if stages else None
        skips = np.zeros((height, width), np.int32) if stages else None
        first = np.zeros(height, np.int32) if stages else None
        every = np.zeros((height, width, int(num_rays), 4), np.float32) if stages else None
        d = orc.Destination(width, height, 1, 1, 1, frame, 1 if progressive else 0, nthreads)
        lib().orc_ao_render(self._h, scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), len(seeds), C.byref(d),
                            int(num_rays), float(radius), int(filter), int(not break_on_terminate), int(stale_isect), _p(self.film),
                            _p(state), _p(value), _p(depth), _p(ray), _p(ans), _p(skips), _p(first), _p(every))
        if not stages:
            return self.film.copy()
        st = dict(state=state, value=value, depth=depth, first_miss=first.astype(np.int64),
                  ray=dict(org=ray[..., 0, :3].copy(), dir=ray[..., 1, :3].copy(), normal_mapped=ray[..., 0, 3] != 0),
                  answer=dict(kind=ans[..., 0].astype(np.int32), t=ans[..., 1].copy(), c=ans[..., 2].copy(),
                              skips=ans[..., 3].astype(np.int32)),
                  answers=dict(kind=every[..., 0].astype(np.int32), t=every[..., 1].copy(), c=every[..., 2].copy(),
                               skips=every[..., 3].astype(np.int32)),
                  skips=skips)
        return self.film.copy(), st
