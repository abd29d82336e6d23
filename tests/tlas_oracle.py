"""ctypes binding of tests/cxx/tlas_oracle.cpp, the CPU twin of the device-built top layer (atn_tlas_rebuild, docs/TLAS.md): the
pinned world-box / Morton arithmetic with oracle/orc_lbvh.h's sort, hierarchy and threading.  TEST INFRASTRUCTURE ONLY: compiled
with g++ into a temporary directory once per session, loaded by tests; the product never imports it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from aten_amd import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "tlas_oracle.cpp")
CXXFLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
_lib = None
_dir = None

LINK_NOT_INNER, LINK_TLAS_BIT, LINK_OFFSET_MASK = 0x80000000, 2, 0x7ffffff0


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.mkdtemp(prefix="tlas_oracle_")
        so = os.path.join(_dir, "libtlas_oracle.so")
        subprocess.check_call(["g++"] + CXXFLAGS + ["-fPIC", "-shared", "-o", so, SRC])
        l = C.CDLL(so)
        vp = C.c_void_p
        l.orc_tlas_build.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, vp, vp]
        l.orc_tlas_check.argtypes = [vp, C.c_uint32]
        _lib = l
    return _lib


def leaf_table(top):
    """The KIND_TLAS leaves of a host-built top layer in its walk order (hit links from node 0): float32 [n, 4], the leaves' four
    payload floats (f0 = objid, f1, f2 = exid bits, f3 = meshid).  Leaves with neither triangle nor nested tree are dropped."""
    top = np.ascontiguousarray(top, L.BVH_NODE)
    rows, i = [], 0
    while i >= 0:
        nd = top[i]
        if (nd["f0"] >= 0 or nd["f1"] >= 0) and nd["f2"] >= 0:
            rows.append([nd["f0"], nd["f1"], nd["f2"], nd["f3"]])
        i = int(nd["hit"])
    return np.array(rows, np.float32).reshape(-1, 4)


def table_objids(table):
    return table[:, 0].astype(np.int32)


def table_lists(table):
    return (np.ascontiguousarray(table[:, 2]).view(np.uint32) & 0x7fff).astype(np.int64)


def local_boxes(fs, table):
    """Per leaf the box of its list's root as the upload lays it into the node image: float32 [n, 6] (min xyz, max xyz).  A list
    whose root is a triangle leaf takes the triangle's vertices."""
    a = fs.arrays
    out = np.zeros((len(table), 6), np.float32)
    for k, ex in enumerate(table_lists(table)):
        root = a["bvh_lists"][int(ex)][0]
        if root["f0"] >= 0 or root["f1"] >= 0:
            v = a["vtx_pos"][a["triangles"][int(root["f1"])]["idx"], :3]
            out[k, :3], out[k, 3:] = v.min(0), v.max(0)
        else:
            out[k, :3], out[k, 3:] = root["boxmin"], root["boxmax"]
    return out


def build(table, objects, matrices, boxes):
    """The twin's top layer: dict(world [n, 6], codes [n] sorted, indices [n], nodes BVH_NODE [2n - 1] in the reference's order)."""
    table = np.ascontiguousarray(table, np.float32).reshape(-1, 4)
    objects = np.ascontiguousarray(objects, L.OBJECT_PARAM)
    matrices = np.ascontiguousarray(matrices, np.float32).reshape(-1, 4, 4)
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    n = len(table)
    assert n >= 1 and len(boxes) == n
    world = np.zeros((n, 6), np.float32)
    codes, idx = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    nodes = np.zeros(2 * n - 1, L.BVH_NODE)
    p = lambda x: C.c_void_p(x.ctypes.data)
    rc = lib().orc_tlas_build(p(table), n, p(objects), len(objects), p(matrices) if len(matrices) else None, len(matrices), p(boxes),
                              p(world), p(codes), p(idx), p(nodes))
    if rc != 0:
        raise ValueError("orc_tlas_build: an id is out of range")
    return dict(world=world, codes=codes, indices=idx, nodes=nodes)


def check(nodes, n_leaves):
    """0, or the number of the structural rule the layer breaks (tlas_oracle.cpp: orc_tlas_check)."""
    nodes = np.ascontiguousarray(nodes, L.BVH_NODE)
    assert len(nodes) == 2 * n_leaves - 1
    return int(lib().orc_tlas_check(C.c_void_p(nodes.ctypes.data), n_leaves))


def scene_with_twin_top(fs, boxes=None):
    """Replaces fs's top layer by the twin's over fs's own objects, matrices and (unless given) list roots; returns the twin."""
    table = leaf_table(fs.arrays["bvh_lists"][0])
    t = build(table, fs.arrays["objects"], fs.arrays["matrices"], local_boxes(fs, table) if boxes is None else boxes)
    t["table"] = table
    fs.replace_bvh_list(0, t["nodes"])
    return t


def decode_records(rec, top_base, n_leaves):
    """Device records (PathTracing.tlas_records) -> per record kind and fields, with links mapped from typed byte offsets to record
    indices (-1 = end).  Returns dict(is_leaf, hit, miss, box [m, 6] float32 bits as uint32, objid, w2l_row, blas_root, flags, meshid, twin)."""
    rec = np.ascontiguousarray(rec, np.uint32).reshape(-1, 8)
    m = len(rec)

    def link(v):
        v = v.astype(np.int64)
        end = v == 0xffffffff
        idx = ((v & LINK_OFFSET_MASK) - top_base) // 32
        return np.where(end, -1, idx), np.where(end, False, (v & LINK_NOT_INNER) != 0)
    # a record is a leaf iff some link (or the root link) names it with the TLAS bit: with the fixed placement, records n-1 .. 2n-2
    is_leaf = np.arange(m) >= n_leaves - 1 if n_leaves > 1 else np.ones(m, bool)
    hit = np.where(is_leaf, link(rec[:, 5])[0], link(rec[:, 3])[0])
    miss = np.where(is_leaf, link(rec[:, 6])[0], link(rec[:, 7])[0])
    return dict(is_leaf=is_leaf, hit=hit, miss=miss, box=rec[:, [0, 1, 2, 4, 5, 6]], objid=rec[:, 0].astype(np.int32),
                w2l_row=rec[:, 1].astype(np.int32), blas_root=rec[:, 2].astype(np.int32), flags=rec[:, 3].astype(np.int32),
                meshid=rec[:, 4].astype(np.int32), twin=rec[:, 7].astype(np.int32))
