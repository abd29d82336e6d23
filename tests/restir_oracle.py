"""ctypes binding of tests/cxx/restir_oracle.cpp, the CPU restatement of the reference's ReSTIR renderer.  TEST INFRASTRUCTURE
ONLY: compiled with g++ into a temporary directory once per session, loaded by tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "restir_oracle.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="restir_oracle_")
        so = os.path.join(_dir, "librestir_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-o", so, SRC])
        l = C.CDLL(so)
        vp = C.c_void_p
        l.orc_restir_create.restype = vp
        l.orc_restir_destroy.argtypes = [vp]
        l.orc_restir_set_motion_depth.argtypes = [vp, vp, C.c_uint32]
        l.orc_restir_set_offset_origin.argtypes = [vp, C.c_int32]
        l.orc_restir_render.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
        l.orc_restir_render.restype = C.c_int
        _lib = l
    return _lib


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class ReSTIR:
    """Frame-persistent ReSTIR state on the CPU (two reservoir / info sets, camera matrices, motion buffer)."""

    def __init__(self):
        self._h = C.c_void_p(lib().orc_restir_create())
        self.film = None

    def close(self):
        if self._h:
            lib().orc_restir_destroy(self._h)
            self._h = None

    def set_offset_origin(self, on):
        """Test switch: visibility rays start at ray::Offset(p, nml) instead of the reference's p + AT_MATH_EPSILON * nml (whose
        rays can hit their own surface -- docs/RESTIR.md)."""
        lib().orc_restir_set_offset_origin(self._h, int(on))

    def set_motion_depth(self, md):
        md = np.ascontiguousarray(md, np.float32).reshape(-1, 4)
        lib().orc_restir_set_motion_depth(self._h, _ptr(md), len(md))

    def render(self, scene, cam, seeds, width, height, max_depth=5, rr_depth=3, frame=0, mode=1, n_candidates=32,
               compute_motion=False, progressive=True, nthreads=0, stages=False):
        """One frame into self.film (kept across calls like the product's film).  Returns the film, and with stages=True a dict:
        initial / temporal / spatial (y, M, W, w_sum, target_pdf), info, nd, am, motion, dims, terminated."""
        if self.film is None or self.film.shape[:2] != (height, width):
            self.film = np.zeros((height, width, 4), np.float32)
        n = width * height
        st = np.zeros((3, height, width, 5), np.float32) if stages else None
        info = np.zeros((4, height, width, 4), np.float32) if stages else None
        aovs = np.zeros((3, height, width, 4), np.float32) if stages else None
        dims = np.zeros((height, width), np.uint32) if stages else None
        term = np.zeros((height, width), np.uint8) if stages else None
        d = orc.Destination(width, height, max_depth, rr_depth, 1, frame, 1 if progressive else 0, nthreads)
        rc = lib().orc_restir_render(self._h, scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), len(seeds),
                                     C.byref(d), mode, n_candidates, int(compute_motion), C.c_void_p(self.film.ctypes.data),
                                     _ptr(st), _ptr(info), _ptr(aovs), _ptr(dims), _ptr(term))
        if rc != 0:
            raise RuntimeError("orc_restir_render: no motion/depth buffer")
        if not stages:
            return self.film.copy()

        def res(k):
            a = st[k]
            return dict(y=a[..., 0].astype(np.int32), M=a[..., 1].astype(np.int32), W=a[..., 2].copy(), w_sum=a[..., 3].copy(),
                        target_pdf=a[..., 4].copy())
        out = dict(initial=res(0), temporal=res(1), spatial=res(2), dims=dims, terminated=term.astype(bool),
                   info=dict(nml=info[0, ..., :3].copy(), mtrl=info[0, ..., 3].copy().view(np.int32), wi=info[1, ..., :3].copy(),
                             u=info[1, ..., 3].copy(), p=info[2, ..., :3].copy(), v=info[2, ..., 3].copy(), pre_r=info[3, ..., 0].copy(),
                             mesh=info[3, ..., 1].copy().view(np.int32), hit=info[3, ..., 2].copy()),
                   nd=aovs[0], am=aovs[1], motion=aovs[2])
        return self.film.copy(), out
