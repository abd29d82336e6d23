"""ctypes binding of tests/cxx/npr_hatching_oracle.cpp, the CPU restatement of the NPR renderer's hatching-shadow filters, and the
hatching pre-pass put together from it, the AO twin (the source plane of the AO base) and the NPR shadow twin (the lit bit, the depth).
TEST INFRASTRUCTURE ONLY: compiled with g++ into a temporary directory once per session, loaded by tests; the product never imports
it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "npr_hatching_oracle.cpp")
NONE, HORIZONTAL, VERTICAL, ORTHOGONAL, CROSS, ORTHOGONAL_CROSS = range(6)      # HatchingShadowDirection
ANTI_DIAGONAL = 6       # the twin's own: OrthogonalCross's second filter alone
AO, SHADOW_RAY = 0, 1   # HatchingShadowBase
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="npr_hatching_oracle_")
        so = os.path.join(_dir, "libnpr_hatching_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so, SRC])
        l = C.CDLL(so)
        vp, i = C.c_void_p, C.c_int32
        l.orc_nprh_filter.argtypes = [i, i, i, vp, vp, vp, vp]
        l.orc_nprh_filter.restype = C.c_int
        _lib = l
    return _lib


def filter(src, depth, direction, first=False):
    """The filter of `direction` (0..5, or ANTI_DIAGONAL) over planes [h, w] -> the final plane; with first=True (final, the first
    step's plane)."""
    s = np.ascontiguousarray(src, np.float32)
    d = np.ascontiguousarray(depth, np.float32)
    assert s.shape == d.shape and s.ndim == 2
    out, one = np.zeros_like(s), np.zeros_like(s)
    rc = lib().orc_nprh_filter(s.shape[1], s.shape[0], int(direction), C.c_void_p(s.ctypes.data), C.c_void_p(d.ctypes.data),
                               C.c_void_p(one.ctypes.data), C.c_void_p(out.ctypes.data))
    assert rc == 0
    return (out, one) if first else out


def flip_class(src, depth, direction, margin=1e-5):
    """Pixels of a two-step direction whose product lies in [1 - margin, 1): a value computed elsewhere within the two-step bound may
    land on the other side of the halving threshold."""
    if direction not in (CROSS, ORTHOGONAL_CROSS):
        return np.zeros(np.shape(src), bool)
    _, a = filter(src, depth, direction, first=True)
    b = filter(src, depth, VERTICAL if direction == CROSS else ANTI_DIAGONAL)
    prod = a.astype(np.float64) * b.astype(np.float64)
    return (prod >= 1.0 - margin) & (prod < 1.0)


def prepass(scene, cam, seeds, width, height, frame=0, base=SHADOW_RAY, direction=HORIZONTAL, num_rays=1, radius=1.0, shadow=None):
    """The hatching pre-pass of one frame -> dict source (the lit bit as 0.0 / 1.0, or the AO values with 1.0 at a primary miss), depth
    (the primary t, inf for a miss), first, plane (the final plane), mtrl, all [h, w].  `shadow`: an npr_shadow_oracle.prepass result of
    the same frame to reuse."""
    import npr_shadow_oracle
    sp = shadow if shadow is not None else npr_shadow_oracle.prepass(scene, cam, seeds, width, height, frame=frame)
    depth = sp["depth"]
    if base == SHADOW_RAY:
        source = sp["lit"]
    else:
        import ao_oracle
        o = ao_oracle.AO()
        try:
            # the AO renderer's own sampler, idaten's miss rule, a fresh intersection record per pixel (docs/NPR_HATCHING.md)
            _, st = o.render(scene, cam, seeds, width, height, num_rays=num_rays, radius=radius, frame=frame, break_on_terminate=False,
                             stale_isect=False, stages=True)
        finally:
            o.close()
        hit = np.isfinite(depth)
        assert np.array_equal(st["state"] == 1, hit)
        assert np.array_equal(st["depth"][hit], depth[hit])
        source = np.where(hit, st["value"], np.float32(1.0)).astype(np.float32)
    plane, first = filter(source, depth, direction, first=True)
    return dict(source=source, depth=depth, first=first, plane=plane, mtrl=sp["mtrl"], lit=sp["lit"])
