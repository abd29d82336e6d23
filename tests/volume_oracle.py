"""ctypes binding of tests/cxx/volume_oracle.cpp, the CPU restatement of the reference's volume path tracer for homogeneous media.
TEST INFRASTRUCTURE ONLY: compiled with g++ into a temporary directory once per session, loaded by tests; the product never imports
it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "volume_oracle.cpp")
_lib = None
_dir = None

FLAGS = dict(processed=1, hit=2, sampled=4, absorbed=8, scattered=16, passed=32, connection=64, visible=128, terminated=256)


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="volume_oracle_")
        so = os.path.join(_dir, "libvolume_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                               "-o", so, SRC])
        l = C.CDLL(so)
        vp, f, i, u = C.c_void_p, C.c_float, C.c_int32, C.c_uint32
        l.orc_vol_render.argtypes = [vp, vp, vp, u, vp, i, vp, i, vp, vp, vp, vp, vp]
        l.orc_vol_render.restype = C.c_int
        l.orc_vol_trace_path.argtypes = [vp, vp, vp, vp, u, u, i, i, vp, vp, vp, vp, vp]
        l.orc_vol_trace_path.restype = i
        l.orc_vol_connect.argtypes = [vp, vp, vp, i, vp, i, vp]
        l.orc_vol_phase_eval.argtypes = [f, u, vp, vp, vp]
        l.orc_vol_phase_sample.argtypes = [f, u, vp, vp, vp, vp]
        l.orc_vol_medium_sample.argtypes = [vp, f, u, vp, vp, vp, vp, vp, vp]
        l.orc_vol_sizeof_medium.restype = u
        _lib = l
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _f(v, shape=None):
    a = np.ascontiguousarray(v, np.float32)
    return a if shape is None else a.reshape(shape)


def sizeof_medium():
    return int(lib().orc_vol_sizeof_medium())


def phase_eval(g, wi, wo):
    wi, wo = _f(wi, (-1, 3)), _f(wo, (-1, 3))
    out = np.zeros(len(wi), np.float32)
    lib().orc_vol_phase_eval(g, len(wi), _p(wi), _p(wo), _p(out))
    return out


def phase_sample(g, w, r1, r2):
    w, r1, r2 = _f(w, (-1, 3)), _f(r1, (-1,)), _f(r2, (-1,))
    out = np.zeros((len(r1), 3), np.float32)
    lib().orc_vol_phase_sample(g, len(r1), _p(w), _p(r1), _p(r2), _p(out))
    return out


def medium_sample(g, sigma_a, sigma_s, le, distance, scramble):
    """HomogeniousMedium::Sample for len(scramble) samplers along +z over `distance` -> dict kind (0 none, 1 absorbed, 2 scattered),
    s, draws, throughput [n, 3], dir [n, 3]."""
    import struct
    med = np.frombuffer(struct.pack("<fffif3f", g, sigma_a, sigma_s, -1, -1.0, *le), np.float32).copy()
    scramble = np.ascontiguousarray(scramble, np.uint32)
    n = len(scramble)
    kind, draws = np.zeros(n, np.int32), np.zeros(n, np.int32)
    s, thr, d = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    lib().orc_vol_medium_sample(_p(med), distance, n, _p(scramble), _p(kind), _p(s), _p(draws), _p(thr), _p(d))
    return dict(kind=kind, s=s, draws=draws, throughput=thr, dir=d)


def unpack_state(raw):
    out = {k: (raw[..., 0] & v) != 0 for k, v in FLAGS.items()}
    out.update(depth_count=raw[..., 1].astype(np.int32), stack_size=raw[..., 2].astype(np.int32), dim=raw[..., 3].copy())
    return out


def unpack_stack(raw):
    """uint32 [..., 4] -> int32 [..., 8] in the order the media were entered."""
    return np.stack([(raw[..., k // 2] >> (16 * (k % 2))) & 0xffff for k in range(8)], axis=-1).astype(np.int32)


def _stages(state, stack, ray, conn):
    st = unpack_state(state)
    return dict(state=st, stack=unpack_stack(stack),
                ray=dict(org=ray[..., 0, :3].copy(), s=ray[..., 0, 3].copy(), dir=ray[..., 1, :3].copy(), hit_t=ray[..., 1, 3].copy()),
                conn=dict(org=conn[..., 0, :3].copy(), t_max=conn[..., 0, 3].copy(), dir=conn[..., 1, :3].copy(),
                          transmittance=conn[..., 1, 3].copy(), segments=conn[..., 2, 0].astype(np.int32), visible=conn[..., 2, 1] != 0))


def trace_path(scene, cam, org, dir, frame=0, rnd=12345, max_depth=5, rr_depth=3):
    """One path by hand through radiance: -> (iterations run, stages dict with a leading axis of 8 iterations, contrib [3])."""
    state, stack = np.zeros((8, 4), np.uint32), np.zeros((8, 4), np.uint32)
    ray, conn = np.zeros((8, 2, 4), np.float32), np.zeros((8, 3, 4), np.float32)
    contrib = np.zeros(3, np.float32)
    o, d = _f(org, (3,)), _f(dir, (3,))
    n = lib().orc_vol_trace_path(scene.ref(), C.c_void_p(cam.ctypes.data), _p(o), _p(d), frame, rnd, max_depth, rr_depth,
                                 _p(state), _p(stack), _p(ray), _p(conn), _p(contrib))
    return int(n), _stages(state, stack, ray, conn), contrib


def connect(scene, start, nml, light_idx=0, stack=()):
    """TraverseRayInMedium from `start` towards light `light_idx` with the medium stack `stack` (material ids, first entered first)
    -> dict visible, transmittance, segments, walk_overflow."""
    out = np.zeros(4, np.float32)
    s, n = _f(start, (3,)), _f(nml, (3,))
    ids = np.ascontiguousarray(stack, np.int32)
    lib().orc_vol_connect(scene.ref(), _p(s), _p(n), light_idx, _p(ids) if len(ids) else None, len(ids), _p(out))
    return dict(visible=bool(out[0]), transmittance=float(out[1]), segments=int(out[2]), walk_overflow=int(out[3]))


class Volume:
    """The film of the CPU volume renderer across progressive frames."""

    def __init__(self):
        self.film = None
        self.counters = None

    def reset(self):
        self.film = None

    def render(self, scene, cam, seeds, width, height, max_depth=5, rr_depth=3, spp=1, frame=0, progressive=True,
               break_on_terminate=True, nthreads=0, capture=None):
        """One frame into self.film.  Returns the film, and with capture = an iteration (0..7) the stage dict of sample 0 after it:
        state, stack [h, w, 8], ray, conn (as PathTracing.volume_buffer).  self.counters: stack_overflow, walk_overflow, connections,
        segments of the frame."""
        if self.film is None or self.film.shape[:2] != (height, width):
            self.film = np.zeros((height, width, 4), np.float32)
        cap = -1 if capture is None else int(capture)
        state = np.zeros((height, width, 4), np.uint32) if cap >= 0 else None
        stack = np.zeros((height, width, 4), np.uint32) if cap >= 0 else None
        ray = np.zeros((height, width, 2, 4), np.float32) if cap >= 0 else None
        conn = np.zeros((height, width, 3, 4), np.float32) if cap >= 0 else None
        cnt = np.zeros(4, np.uint64)
        d = orc.Destination(width, height, max_depth, rr_depth, spp, frame, 1 if progressive else 0, nthreads)
        lib().orc_vol_render(scene.ref(), C.c_void_p(cam.ctypes.data), C.c_void_p(seeds.ctypes.data), len(seeds), C.byref(d),
                             int(break_on_terminate), _p(self.film), cap, _p(state), _p(stack), _p(ray), _p(conn), _p(cnt))
        self.counters = dict(stack_overflow=int(cnt[0]), walk_overflow=int(cnt[1]), connections=int(cnt[2]), segments=int(cnt[3]))
        if cap < 0:
            return self.film.copy()
        return self.film.copy(), _stages(state, stack, ray, conn)
