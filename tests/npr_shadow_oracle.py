"""ctypes binding of tests/cxx/npr_shadow_oracle.cpp, the CPU restatement of the NPR renderers' screen-space shadow pre-pass.  TEST
INFRASTRUCTURE ONLY: compiled with g++ into a temporary directory once per session, loaded by tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "npr_shadow_oracle.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="npr_shadow_oracle_")
        so = os.path.join(_dir, "libnpr_shadow_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-o", so, SRC])
        l = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int32
        l.orc_nprs_filter.argtypes = [i, i, vp, vp, vp]
        l.orc_nprs_prepass.argtypes = [vp, vp, vp, C.c_uint32, vp, vp, vp, vp, vp]
        l.orc_nprs_prepass.restype = C.c_int
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def row_filter(lit, depth):
    """ApplyBilateralFilter<ShadowRay, float, true, 5> with coefficients (2, 2) over planes [h, w] -> the filtered plane."""
    l = np.ascontiguousarray(lit, np.float32)
    d = np.ascontiguousarray(depth, np.float32)
    assert l.shape == d.shape and l.ndim == 2
    out = np.zeros_like(l)
    lib().orc_nprs_filter(l.shape[1], l.shape[0], _p(l), _p(d), _p(out))
    return out


def prepass(scene, cam, seeds, width, height, frame=0, max_depth=5, rr_depth=3, nthreads=0):
    """The pre-pass of one frame -> dict lit (0.0 / 1.0), depth (the primary t, inf for a miss), plane (filtered), mtrl (the primary
    hit's material id, -1 for a miss), all [h, w]."""
    lit = np.zeros((height, width), np.float32)
    depth = np.zeros((height, width), np.float32)
    plane = np.zeros((height, width), np.float32)
    mtrl = np.zeros((height, width), np.int32)
    d = orc.Destination(width, height, max_depth, rr_depth, 1, frame, 1, nthreads)
    rc = lib().orc_nprs_prepass(scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), len(seeds), C.byref(d),
                                _p(lit), _p(depth), _p(plane), _p(mtrl))
    assert rc == 0
    return dict(lit=lit, depth=depth, plane=plane, mtrl=mtrl)


def plug_plane(scene, plane):
    """Points a BUILT scene's screen_space_texture at `plane` [h, w] (x channel; context::GetScreenSpaceTextureAt), so that orc.render
    and npr_oracle.NPR.render of the scene are the frame references of a mode-1 frame.  plane=None unplugs it.  The scene keeps the
    array alive."""
    d = scene.desc
    if plane is None:
        d.screen_space_texture.texels = None
        d.screen_space_texture.width = d.screen_space_texture.height = 0
        scene.keep.append(None)
        return scene
    sst = np.zeros(plane.shape + (4,), np.float32)
    sst[..., 0] = plane
    d.screen_space_texture.texels = sst.ctypes.data
    d.screen_space_texture.height, d.screen_space_texture.width = sst.shape[0], sst.shape[1]
    scene.keep.append(sst)
    return scene
