"""ctypes binding of tests/cxx/npr_advance_oracle.cpp: the NPR oracle with AdvanceNPRPath (the look-through of STENCIL and alpha
surfaces) restated literally.  TEST INFRASTRUCTURE ONLY: compiled with g++ into a temporary directory once per session, loaded by
tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "npr_advance_oracle.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="npr_advance_oracle_")
        so = os.path.join(_dir, "libnpr_advance_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-o", so, SRC])
        l = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int32
        l.orc_npr_create.restype = vp
        l.orc_npr_destroy.argtypes = [vp]
        l.orc_npr_reset.argtypes = [vp]
        l.orc_npra_render.argtypes = [vp, vp, vp, vp, C.c_uint32, vp, i, vp, vp, vp, vp, vp, vp, vp]
        l.orc_npra_render.restype = C.c_int
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


class NPRAdvance:
    """Frame-persistent NPR state on the CPU (tests/npr_oracle.py's NPR), every frame rendered with the advance."""

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
               break_on_terminate=True, nthreads=0, stages=False):
        """One frame into self.film.  Returns the film, and with stages=True a dict: npr_oracle's line, desc, terminated, disc, dims,
        and adv: kind, walks, answer, singular, throughput, transmission (PathTracing.npr_advance_buffer's) with verdict (CheckStencil:
        0 not STENCIL, 1 true, 2 back-facing ALWAYS, 3 NONE, 4 miss, 5 ten layers), alpha_end (0 none, 1 opaque hit, 2 miss, 3 the tenth
        walk ended on a pane), rewalk_same (the literal re-walk gave the last walk's answer) and mtrl (the primary hit's material)."""
        if self.film is None or self.film.shape[:2] != (height, width):
            self.film = np.zeros((height, width, 4), np.float32)
        line = np.zeros((height, width, 4), np.float32) if stages else None
        desc = np.zeros((height, width, 8, 4), np.float32) if stages else None
        disc = np.zeros((height, width, 2, 4), np.float32) if stages else None
        dims = np.zeros((height, width), np.uint32) if stages else None
        adv = np.zeros((height, width, 2, 4), np.float32) if stages else None
        cat = np.zeros((height, width, 4), np.float32) if stages else None
        d = orc.Destination(width, height, max_depth, rr_depth, spp, frame, 1 if progressive else 0, nthreads)
        lib().orc_npra_render(self._h, scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), len(seeds), C.byref(d),
                              int(break_on_terminate), _p(self.film), _p(line), _p(desc), _p(disc), _p(dims), _p(adv), _p(cat))
        if not stages:
            return self.film.copy()
        st = dict(line=dict(found=line[..., 0] != 0, bounce=line[..., 1].astype(np.int32), distance=line[..., 2].copy()),
                  desc=dict(u=desc[..., 0].copy(), v=desc[..., 1].copy(), live=desc[..., 2] != 0),
                  terminated=desc[..., 0, 3] != 0,
                  disc=dict(center=disc[..., 0, :3].copy(), radius=disc[..., 0, 3].copy(), normal=disc[..., 1, :3].copy(),
                            acc=disc[..., 1, 3].copy()),
                  dims=dims,
                  adv=dict(kind=adv[..., 0, 0].astype(np.int32), walks=adv[..., 0, 1].astype(np.int32), answer=adv[..., 0, 2].astype(np.int32),
                           singular=adv[..., 0, 3] != 0, throughput=adv[..., 1, :3].copy(), transmission=adv[..., 1, 3].copy(),
                           verdict=cat[..., 0].astype(np.int32), alpha_end=cat[..., 1].astype(np.int32), rewalk_same=cat[..., 2] != 0,
                           mtrl=cat[..., 3].astype(np.int32)))
        return self.film.copy(), st
