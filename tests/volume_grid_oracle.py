"""ctypes binding of tests/cxx/volume_grid_oracle.cpp: the CPU twin of the volume renderer with grid media (tests/cxx/volume_oracle.cpp
plus the grid branches; the tracking loops are the product's own aten_amd/csrc/device/volume_grid_track.h).  TEST INFRASTRUCTURE ONLY:
compiled with g++ into a temporary directory once per session."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import orc
from volume_oracle import _f, _p, _stages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "volume_grid_oracle.cpp")
_lib = None

KINDS = dict(miss=0, end=1, scatter=2, capped=3)


class Grid(C.Structure):
    """atn_volume_grid (include/aten_amd.h)."""
    _fields_ = [("dim", C.c_int32 * 3), ("origin", C.c_float * 3), ("voxel_size", C.c_float), ("density", C.c_void_p)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="volume_grid_oracle_")
        so = os.path.join(d, "libvolume_grid_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-o", so, SRC])
        l = C.CDLL(so)
        vp, f, i, u = C.c_void_p, C.c_float, C.c_int32, C.c_uint32
        l.orc_vol_render.argtypes = [vp, vp, vp, u, vp, i, vp, i, vp, vp, vp, vp, vp, vp, u, vp]
        l.orc_vol_render.restype = C.c_int
        l.orc_volg_delta_track.argtypes = [vp, f, f, f, vp, vp, f, u, u, vp, vp, vp, vp, vp, vp, vp, u, vp, vp, vp]
        l.orc_volg_ratio_track.argtypes = [vp, f, f, f, vp, vp, f, u, u, vp, vp, vp, vp]
        _lib = l
    return _lib


def pack_grids(grids):
    """[(density [z, y, x], origin, voxel_size)] -> (atn_volume_grid array, the arrays it points into)."""
    arr = (Grid * max(1, len(grids)))()
    keep = []
    for k, (density, origin, voxel_size) in enumerate(grids):
        d = np.ascontiguousarray(density, np.float32)
        keep.append(d)
        arr[k].dim[:] = [d.shape[2], d.shape[1], d.shape[0]]
        arr[k].origin[:] = [float(c) for c in origin]
        arr[k].voxel_size = float(voxel_size)
        arr[k].density = d.ctypes.data
    return arr, keep


def delta_track(grid, sigma_s, majorant, org, dir, t_surface, scramble, sigma_a=0.0, log=0, dim=2):
    """HeterogeneousMedium::Sample along org + t * dir over [0, t_surface] for len(scramble) streams (index i % 256, dimension `dim`) ->
    dict kind (KINDS), s, steps, draws, factor, tie; with log = n also log_draws [2 n], log_s [n], log_idx [n, 3] of stream 0."""
    arr, keep = pack_grids([grid])
    scramble = np.ascontiguousarray(scramble, np.uint32)
    n = len(scramble)
    kind, steps, draws, tie = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    s, factor = np.zeros(n, np.float32), np.zeros(n, np.float32)
    ld, ls, li = np.zeros(2 * max(log, 1), np.float32), np.zeros(max(log, 1), np.float32), np.zeros((max(log, 1), 3), np.float32)
    o, d = _f(org, (3,)), _f(dir, (3,))
    lib().orc_volg_delta_track(C.byref(arr), sigma_a, sigma_s, majorant, _p(o), _p(d), t_surface, n, dim, _p(scramble), _p(kind), _p(s), _p(steps),
                               _p(draws), _p(factor), _p(tie), log, _p(ld), _p(ls), _p(li))
    return dict(kind=kind, s=s, steps=steps, draws=draws, factor=factor, tie=tie != 0, log_draws=ld, log_s=ls, log_idx=li)


def ratio_track(grid, sigma_s, majorant, org, dir, distance, scramble, sigma_a=0.0, dim=2):
    """HeterogeneousMedium::EvaluateTransmittance over [0, distance] for len(scramble) connection streams -> dict tr, steps, capped."""
    arr, keep = pack_grids([grid])
    scramble = np.ascontiguousarray(scramble, np.uint32)
    n = len(scramble)
    tr, steps, capped = np.zeros(n, np.float32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    o, d = _f(org, (3,)), _f(dir, (3,))
    lib().orc_volg_ratio_track(C.byref(arr), sigma_a, sigma_s, majorant, _p(o), _p(d), distance, n, dim, _p(scramble), _p(tr), _p(steps), _p(capped))
    return dict(tr=tr, steps=steps, capped=capped != 0)


class Volume:
    """The film of the CPU volume renderer with grid media across progressive frames (volume_oracle.Volume with `grids`)."""

    def __init__(self):
        self.film = None
        self.counters = None

    def reset(self):
        self.film = None

    def render(self, scene, cam, seeds, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, progressive=True,
               break_on_terminate=True, nthreads=0, capture=None, grids=None):
        """As volume_oracle.Volume.render; grids defaults to scene.grids.  With capture the stage dict also has state flight_steps,
        conn track_steps / stream_dim, and ties: uint32 [h, w], 1 = the flight, 2 = the connection lay within 1e-5 of another
        decision.  self.counters adds flight_capped and connection_capped."""
        if self.film is None or self.film.shape[:2] != (height, width):
            self.film = np.zeros((height, width, 4), np.float32)
        grids = list(getattr(scene, "grids", [])) if grids is None else list(grids)
        arr, keep = pack_grids(grids)
        cap = -1 if capture is None else int(capture)
        state = np.zeros((height, width, 4), np.uint32) if cap >= 0 else None
        stack = np.zeros((height, width, 4), np.uint32) if cap >= 0 else None
        ray = np.zeros((height, width, 2, 4), np.float32) if cap >= 0 else None
        conn = np.zeros((height, width, 3, 4), np.float32) if cap >= 0 else None
        ties = np.zeros((height, width), np.uint32) if cap >= 0 else None
        cnt = np.zeros(6, np.uint64)
        d = orc.Destination(width, height, max_depth, rr_depth, spp, frame, 1 if progressive else 0, nthreads)
        lib().orc_vol_render(scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), len(seeds), C.byref(d),
                             int(break_on_terminate), _p(self.film), cap, _p(state), _p(stack), _p(ray), _p(conn), _p(cnt),
                             C.byref(arr), len(grids), _p(ties))
        self.counters = dict(stack_overflow=int(cnt[0]), walk_overflow=int(cnt[1]), connections=int(cnt[2]), segments=int(cnt[3]),
                             flight_capped=int(cnt[4]), connection_capped=int(cnt[5]))
        if cap < 0:
            return self.film.copy()
        st = _stages(state, stack, ray, conn)
        st["state"]["flight_steps"] = ((state[..., 0] >> 16) & 0x7fff).astype(np.int32)
        st["conn"]["track_steps"] = conn[..., 2, 2].astype(np.int32)
        st["conn"]["stream_dim"] = conn[..., 2, 3].astype(np.int32)
        st["ties"] = ties
        st["raw"] = dict(state=state, stack=stack, ray=ray, conn=conn)
        return self.film.copy(), st
