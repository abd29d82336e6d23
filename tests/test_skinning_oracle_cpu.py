"""Skinning on the CPU: the twin (tests/cxx/skinning_oracle.cpp) against a float64 evaluation and exact cases, the 72-byte record,
the scene's skinned tube, and the library's new entry points."""
import os
import re
import subprocess

import numpy as np

import skinning_oracle as S
from aten_amd import layout as L
from conftest import ulp_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atn_skin_create", "atn_skin_update", "atn_skin_compute", "atn_lbvh_rebuild_list_skinned", "atn_skin_download",
         "atn_skin_download_list", "atn_skin_destroy")
EPS = float(np.finfo(np.float32).eps)


def fan(n, vtx_offset=0):
    """max(n // 3, 0) triangles over vertices (3 i, 3 i + 1, 3 i + 2), as the builder lays a mesh out."""
    t = np.zeros(n // 3, L.TRIANGLE_PARAM)
    t["idx"] = vtx_offset + np.arange(3 * (n // 3), dtype=np.int32).reshape(-1, 3)
    return t


def f64_skin(v, m):
    """computeSkinning in float64 from the float32 inputs: (positions, unnormalised normals as vec4, sum of |terms| per component)."""
    m = m.astype(np.float64)
    p = v["position"].astype(np.float64)
    n = np.concatenate([v["normal"].astype(np.float64), np.zeros((len(v), 1))], 1)
    bi = v["blend_index"].astype(np.int64)
    w = v["blend_weight"].astype(np.float64)
    rp, rn, mag_p, mag_n = np.zeros((len(v), 4)), np.zeros((len(v), 4)), np.zeros((len(v), 4)), np.zeros((len(v), 4))
    for b in range(4):
        W = w[:, b, None, None] * m[bi[:, b]]
        rp += np.einsum("nij,nj->ni", W, p); rn += np.einsum("nij,nj->ni", W, n)
        mag_p += np.einsum("nij,nj->ni", np.abs(W), np.abs(p)); mag_n += np.einsum("nij,nj->ni", np.abs(W), np.abs(n))
    return rp, rn, mag_p, mag_n


# ---- 1. symbols and layout ------------------------------------------------------------------------------------------------------
def test_library_exports_skinning_entry_points():
    from aten_amd import _lib
    so = os.environ.get("ATEN_AMD_LIB") or os.path.join(ROOT, "aten_amd", "libaten_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    for s in NAMES:
        assert s in _lib.SYMBOLS
        assert s in names, s
        assert re.search(r"^int %s\(atn_ctx\* ctx" % s, header, re.M), s
    assert "atn_skinning_vertex" in open(os.path.join(ROOT, "include", "aten_layout.h")).read()


def test_skinning_vertex_layout():
    d = L.SKINNING_VERTEX
    assert d.itemsize == 72 == S.lib().orc_skin_sizeof_vertex()
    assert [d.fields[k][1] for k in ("position", "normal", "clr", "uv", "blend_index", "blend_weight")] == [0, 16, 28, 32, 40, 56]


# ---- 2. the twin's arithmetic ---------------------------------------------------------------------------------------------------
def test_twin_matches_float64_within_fp32_rounding():
    # Every output component is a sum of 16 terms weight * matrix entry * coordinate; a term passes through at most 2 products,
    # 3 additions of its row and 4 of the accumulation = 9 roundings of eps / 2 each: |error| <= 4.5 eps * sum|terms| to first
    # order.  5 eps is used.
    v, m = S.random_vertices(5000, 37, 1), S.random_palette(37, 2)
    t = S.SkinTwin(v).compute(m, True)
    rp, rn, mag_p, mag_n = f64_skin(v, m)
    assert np.all(np.abs(t.pos[:, :3] - rp[:, :3]) <= 5 * EPS * mag_p[:, :3])
    # the normal x / |v|: the same bound on x, the errors of all four components in |v| (|x| / |v| <= 1), and the normalisation's
    # own roundings (4 squares and 3 additions halved by the sqrt, the sqrt, the reciprocal, the product: < 3 eps)
    ln = np.sqrt((rn * rn).sum(1, keepdims=True))
    assert np.all(np.abs(t.nml[:, :3] - (rn / ln)[:, :3]) <= (5 * EPS * mag_n[:, :3] + 5 * EPS * mag_n.sum(1, keepdims=True) + 3 * EPS * np.abs(rn[:, :3])) / ln)
    assert np.array_equal(t.pos[:, 3], v["uv"][:, 0]) and np.array_equal(t.nml[:, 3], v["uv"][:, 1])


def test_single_bone_identity_and_exact_translation():
    v = S.random_vertices(1000, 3, 3)
    v["blend_weight"] = [1.0, 0.0, 0.0, 0.0]
    ident = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    t = S.SkinTwin(v).compute(ident, True)
    assert t.pos[:, :3].tobytes() == v["position"][:, :3].tobytes()          # the rest pose, bit for bit
    # positions on a grid of 1/256 moved by multiples of 1/256: every product and sum is exact
    v["position"][:, :3] = np.round(v["position"][:, :3] * 256) / 256
    m = ident.copy()
    m[:, :3, 3] = np.array([[0.25, -0.5, 1.0], [3 / 256, 0.0, -7 / 256], [2.0, 2.0, 2.0]], np.float32)
    t = S.SkinTwin(v).compute(m, True)
    want = v["position"][:, :3] + m[v["blend_index"][:, 0].astype(int), :3, 3]
    assert t.pos[:, :3].tobytes() == want.astype(np.float32).tobytes()


def test_rotation_keeps_unit_normals():
    v = S.random_vertices(4000, 1, 4)
    v["blend_weight"] = [1.0, 0.0, 0.0, 0.0]
    a = 0.7
    R = np.eye(4, dtype=np.float32)
    R[0, 0] = R[1, 1] = np.cos(a); R[0, 1] = -np.sin(a); R[1, 0] = np.sin(a)
    t = S.SkinTwin(v).compute(R[None], True)
    # the length of the fp32 normal, taken exactly (float64) and expressed as the fp32 number nearest to it, is 1 to one fp32 ulp
    ln = np.linalg.norm(t.nml[:, :3].astype(np.float64), axis=1).astype(np.float32)
    print("max |normal| - 1 in ulps:", int(ulp_diff(ln, np.ones_like(ln)).max()))
    assert np.all(ulp_diff(ln, np.ones_like(ln)) <= 1)


def test_prev_on_restart_and_after():
    v, m0, m1 = S.random_vertices(300, 5, 5), S.random_palette(5, 6), S.random_palette(5, 7)
    t = S.SkinTwin(v).compute(m0, True)
    assert t.prev[:, :3].tobytes() == t.pos[:, :3].tobytes() and np.all(t.prev[:, 3] == 1.0)
    p0 = t.pos.copy()
    t.compute(m1, False)
    assert t.prev[:, :3].tobytes() == p0[:, :3].tobytes() and np.all(t.prev[:, 3] == 1.0)
    assert t.pos.tobytes() != p0.tobytes()
    t.compute(m1, True)
    assert t.prev[:, :3].tobytes() == t.pos[:, :3].tobytes()


def test_area_is_the_unhalved_cross_length():
    n = 3000
    v, m = S.random_vertices(n, 9, 8), S.random_palette(9, 9)
    t = S.SkinTwin(v, fan(n, 40), vtx_offset=40).compute(m, True)
    p = t.pos[:, :3].astype(np.float64).reshape(-1, 3, 3)
    want = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    # edges, 6 products, 3 differences, 3 squares, 2 sums, a sqrt: a few eps of |e1| |e2|
    scale = np.linalg.norm(p[:, 1] - p[:, 0], axis=1) * np.linalg.norm(p[:, 2] - p[:, 0], axis=1)
    assert np.all(np.abs(t.area - want) <= 8 * EPS * scale)
    assert np.median(t.area / want) > 0.999        # |cross|, not |cross| / 2


def test_bbox_is_min_max_of_the_positions():
    v, m = S.random_vertices(2500, 4, 10), S.random_palette(4, 11)
    t = S.SkinTwin(v).compute(m, True)
    assert np.array_equal(t.bbox[:3], t.pos[:, :3].min(0)) and np.array_equal(t.bbox[3:], t.pos[:, :3].max(0))
    one = S.SkinTwin(v[:1]).compute(m, True)
    assert np.array_equal(one.bbox[:3], one.pos[0, :3]) and np.array_equal(one.bbox[3:], one.pos[0, :3])


# ---- 3. the scene ---------------------------------------------------------------------------------------------------------------
def test_skinned_room_vertices_follow_the_scene_layout():
    from aten_amd.scene import scenedefs
    b, oid, cam, sv = scenedefs.skinned_room(16, 8, 4)
    fs = b.build()
    o = fs.arrays["objects"][oid]
    tr = fs.arrays["triangles"][int(o["triangle_id"]):int(o["triangle_id"]) + int(o["triangle_num"])]
    v0 = int(tr["idx"].min())
    assert len(tr) == 2 * 16 * 8 and len(sv) == 3 * len(tr) == int(tr["idx"].max()) + 1 - v0
    assert sv.dtype == L.SKINNING_VERTEX
    nz = (sv["blend_weight"] > 0).sum(1)
    assert nz.min() == 1 and nz.max() >= 3 and (nz == 1).any()
    assert sv["blend_index"].min() >= 0 and sv["blend_index"].max() <= 3
    # an identity palette returns the uploaded rest pose (w = uv), whatever the weights: they sum to 1 within rounding
    t = S.SkinTwin(sv, tr, vtx_offset=v0).compute(np.tile(np.eye(4, dtype=np.float32), (4, 1, 1)), True)
    assert np.array_equal(t.pos[:, 3], fs.arrays["vtx_pos"][v0:v0 + len(sv), 3])
    # (the fp32 weights sum to 1 within 2 eps, the sums add 4.5 eps: 8 eps of coordinates below 2)
    assert np.abs(t.pos[:, :3] - fs.arrays["vtx_pos"][v0:v0 + len(sv), :3]).max() <= 8 * EPS * 2
    pal = scenedefs.skinned_pose(0.8, 4)
    assert pal.shape == (4, 4, 4) and pal.dtype == np.float32
    t.compute(pal, False)
    assert np.all(t.bbox[:3] > -1.0) and np.all(t.bbox[3:] < 2.0)       # the posed tube stays inside the room
