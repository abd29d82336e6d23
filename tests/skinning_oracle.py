"""ctypes binding of tests/cxx/skinning_oracle.cpp, the CPU twin of the device skinning (the reference's computeSkinning /
setTriangleParam / getMinMax with libaten's host arithmetic).  TEST INFRASTRUCTURE ONLY: compiled with g++ into a temporary
directory once per session, loaded by tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from aten_amd import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "skinning_oracle.cpp")
_lib = None
_dir = None


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="skinning_oracle_")
        so = os.path.join(_dir, "libskinning_oracle.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so, SRC])
        l = C.CDLL(so)
        vp = C.c_void_p
        l.orc_skin_compute.argtypes = [vp, C.c_uint32, vp, C.c_int32, vp, vp, vp, vp, C.c_uint32, vp]
        l.orc_skin_compute.restype = None
        l.orc_skin_sizeof_vertex.restype = C.c_uint32
        _lib = l
    return _lib


class SkinTwin:
    """One idaten::Skinning on the CPU: compute(palette, restart) advances pos / nml / prev / the triangles' areas / bbox by a
    tick.  `triangles` (layout.TRIANGLE_PARAM) hold scene-wide vertex indices; vtx_offset is the skin's first vertex."""

    def __init__(self, vertices, triangles=None, vtx_offset=0, pos0=None):
        self.v = np.ascontiguousarray(vertices, L.SKINNING_VERTEX)
        n = len(self.v)
        self.pos = np.zeros((n, 4), np.float32) if pos0 is None else np.ascontiguousarray(pos0, np.float32).reshape(n, 4).copy()
        self.nml = np.zeros((n, 4), np.float32)
        self.prev = np.zeros((n, 4), np.float32)
        self.bbox = np.zeros(6, np.float32)
        self.vtx_offset = vtx_offset
        self.tris = np.zeros(0, L.TRIANGLE_PARAM) if triangles is None else np.ascontiguousarray(triangles, L.TRIANGLE_PARAM).copy()
        if len(self.tris):
            rel = self.tris["idx"].astype(np.int64) - vtx_offset
            assert rel.min() >= 0 and rel.max() < n

    def compute(self, palette, restart):
        m = np.ascontiguousarray(palette, np.float32).reshape(-1, 4, 4)
        bi = self.v["blend_index"].astype(np.int32)
        assert bi.min() >= 0 and bi.max() < len(m)
        t = self.tris.copy()
        t["idx"] -= self.vtx_offset
        p = lambda a: C.c_void_p(a.ctypes.data)
        lib().orc_skin_compute(p(self.v), len(self.v), p(m), int(bool(restart)), p(self.pos), p(self.nml), p(self.prev),
                               p(t), len(t), p(self.bbox))
        self.tris["area"] = t["area"]
        return self

    @property
    def area(self):
        return self.tris["area"].copy()


def random_vertices(n, n_matrices, seed):
    """n SkinningVertex records: positions in a unit box around (0.3, 1, 0.3), unit normals, one to four bones per vertex with
    weights summing to ~1 (zero weights keep a valid index: all four matrices are read), blend indices in [0, n_matrices)."""
    rng = np.random.default_rng(seed)
    v = np.zeros(n, L.SKINNING_VERTEX)
    v["position"][:, :3] = (rng.random((n, 3)) - 0.5 + np.array([0.3, 1.0, 0.3])).astype(np.float32)
    v["position"][:, 3] = 1.0
    nm = rng.normal(size=(n, 3))
    v["normal"] = (nm / np.linalg.norm(nm, axis=1, keepdims=True)).astype(np.float32)
    v["clr"] = rng.integers(0, 256, (n, 4))
    v["uv"] = rng.random((n, 2)).astype(np.float32)
    v["blend_index"] = rng.integers(0, n_matrices, (n, 4)).astype(np.float32)
    w = rng.random((n, 4))
    w[rng.random((n, 4)) < 0.3] = 0.0
    w[:, 0] += 1e-3
    v["blend_weight"] = (w / w.sum(1, keepdims=True)).astype(np.float32)
    return v


def random_palette(n_matrices, seed):
    """Rigid motions (a rotation about a random axis by up to ~0.5 rad, a translation of up to 0.1) as float32 [n, 4, 4]."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_matrices, 4, 4), np.float32)
    for j in range(n_matrices):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        a = rng.uniform(-0.5, 0.5)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
        M = np.eye(4); M[:3, :3] = R; M[:3, 3] = rng.uniform(-0.1, 0.1, 3)
        out[j] = M.astype(np.float32)
    return out
