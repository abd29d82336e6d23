"""NPR feature lines on the CPU: the twin's geometry (tests/cxx/npr_oracle.cpp, feature_line.h) against hand-worked cases, the
two-pass switch against the one-pass frame, an oracle-free check that lines sit on edges, the typed ABI structs, the builder's
bytes and the library's new entry points."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import npr_oracle as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.lib()
    return o


def test_pixel_width(orc):
    """Camera::ComputePixelWidthAtDistance: vfov 60, 1280 x 720, d = 1 -- the "hfov" is vfov * H / W = 33.75 degrees."""
    cam = orc.create_camera((0, 0, 0), (0, 0, -1), 60.0, 1280, 720)
    assert N.pixel_width(cam, 1.0) == pytest.approx(0.000473979220, rel=1e-6)
    assert N.pixel_width(cam, -2.0) == pytest.approx(2 * 0.000473979220, rel=1e-6)


def test_first_disc():
    """GenerateDisc: centred one unit along the query ray, facing along it, radius = line width x pixel width, accumulated 0."""
    d = N.generate_disc((1, 2, 3), (0, 0, -1), 2.0, 0.5)
    np.testing.assert_allclose(d[:3], (1, 2, 2), atol=1e-6)
    assert d[3] == pytest.approx(1.0)
    np.testing.assert_allclose(d[4:7], (0, 0, -1))
    assert d[7] == 0.0
    # a disc point lies on the disc's plane, `radius` from the centre for (u, v) on the unit circle
    p = N.disc_position(0.6, 0.8, d)
    assert p[2] == pytest.approx(2.0, abs=1e-6)
    assert np.linalg.norm(p - d[:3]) == pytest.approx(1.0, rel=1e-5)


def test_disc_at_query_hit():
    """ComputeDiscAtQueryRayHitPoint: the radius grows with the accumulated distance, the normal faces back along the query ray."""
    d = N.disc_at((0, 0, -5), (0, 0, -1), 0.01, 4.0, 1.0)
    np.testing.assert_allclose(d[:3], (0, 0, -5))
    assert d[3] == pytest.approx(0.05)
    np.testing.assert_allclose(d[4:7], (0, 0, 1))
    assert d[7] == 1.0


def test_plane_hit_and_projection():
    hit, p = N.plane_hit((0, 1, 0), (0, -1, 0), (0, 1, 0), (0, -1, 0))
    assert hit and np.allclose(p, (0, -1, 0))
    hit, _ = N.plane_hit((0, 1, 0), (0, -1, 0), (0, 1, 0), (0, 1, 0))           # behind the origin: t < 0
    assert not hit
    hit, _ = N.plane_hit((0, 1, 0), (0, -1, 0), (0, 1, 0), (1, 0, 0))           # parallel: div == 0
    assert not hit
    dist, y, along = N.project((3, 4, -10), (0, 0, 0), (0, 0, -1))
    assert dist == pytest.approx(5.0) and np.allclose(y, (0, 0, -10)) and along == pytest.approx(10.0)


def test_next_sample_ray_rules():
    prev = N.generate_disc((0, 0, 0), (0, 0, -1), 1.0, 0.01)
    nxt = N.disc_at((0, 0, -4), (0, 0, -1), prev[3], 4.0, 1.0)                  # faces +z: against the previous disc
    # from a hit on a wall facing the camera (+z normal), towards the next disc: allowed, origin offset along the normal
    r = N.next_ray(0.5, 0.0, (0, 0, -2), (0, 0, 1), prev, nxt)
    assert r is None                                                             # the next disc lies behind the wall's normal: dropped
    r = N.next_ray(0.5, 0.0, (0, 0, -2), (0, 0, -1), prev, nxt)
    assert r is not None
    org, d = r
    assert org[2] < -2.0 and np.linalg.norm(d) == pytest.approx(1.0, rel=1e-6)
    # consecutive discs facing away from each other mirror u: the target is -u on the next disc
    target = N.disc_position(-0.5, 0.0, nxt)
    want = (target - np.float32((0, 0, -2))) / np.linalg.norm(target - np.float32((0, 0, -2)))
    np.testing.assert_allclose(d, want, atol=1e-5)
    same = nxt.copy(); same[4:7] = (0, 0, -1)                                   # facing the same way: u kept
    _, d2 = N.next_ray(0.5, 0.0, (0, 0, -2), (0, 0, -1), prev, same)
    t2 = N.disc_position(0.5, 0.0, same)
    np.testing.assert_allclose(d2, (t2 - np.float32((0, 0, -2))) / np.linalg.norm(t2 - np.float32((0, 0, -2))), atol=1e-5)


def test_depth_threshold():
    """t_depth = 2 * max(dq, ds) * |ps - pq| / |dot(pq, n_closest)|, FLT_MAX when the divisor is 0."""
    t = N.depth_threshold((0, 0, 0), 2.0, (0, 0, -4), (0, 0, 1), (1, 0, -4), (0, 0, 1), 4.0, 4.123)
    assert t == pytest.approx(2 * 4.123 * 1.0 / 4.0, rel=1e-6)
    # n_closest is the normal at the nearer point: the sample's here, perpendicular to p->q
    t = N.depth_threshold((0, 0, 0), 2.0, (0, 0, -4), (0, 0, 1), (0, 0, -1), (1, 0, 0), 4.0, 1.0)
    assert t == np.finfo(np.float32).max


def test_line_width():
    """IsInLineWidth: the distance from the query ray against (accumulated + distance along the ray) x pixel width x line width."""
    pw = 0.001
    assert N.in_line_width(2.0, (0, 0, 0), (0, 0, -1), (0.0099, 0, -5), 0.0, pw)           # 5 * 0.001 * 2 = 0.01
    assert not N.in_line_width(2.0, (0, 0, 0), (0, 0, -1), (0.0101, 0, -5), 0.0, pw)
    assert N.in_line_width(2.0, (0, 0, 0), (0, 0, -1), (0.0101, 0, -5), 1.0, pw)            # (1 + 5) * 0.001 * 2 = 0.012


@pytest.mark.parametrize("flag", ["mesh", "albedo", "normal", "depth"])
def test_metric_flags(flag):
    """Each FeatureLineMetricFlag finds its own kind of edge and nothing else; flags 0 find none.  The depth metric compares
    depths from the CAMERA against a threshold built from the query ray's ORIGIN p: since |dq - ds| <= |ps - pq| it can only fire
    where p is not the camera -- a bounce behind the primary hit (here p is 104 units above the query point, the camera at 0)."""
    bit = dict(mesh=1, albedo=2, normal=4, depth=8)[flag]
    p = (0, 0, 100)
    base_q = ((0, 0, -4), (0, 0, 1), 3)
    grey = (0.5, 0.5, 0.5, 1.0)
    cases = dict(mesh=(((0.1, 0, -4), (0, 0, 1), 4), grey, 4.0, 4.0),
                 albedo=(((0.1, 0, -4), (0, 0, 1), 3), (0.9, 0.9, 0.9, 1.0), 4.0, 4.0),
                 normal=(((0.1, 0, -4), (1, 0, 0), 3), grey, 4.0, 4.0),
                 depth=(((0.1, 0, -4.5), (0, 0, 1), 3), grey, 4.0, 4.5))
    # from the camera itself the depth metric never fires: threshold >= 2 |ps - pq| >= 2 |dq - ds|
    assert not N.metrics((0, 0, 0), base_q, ((0.1, 0, -9), (0, 0, 1), 3), grey, grey, 0.1, 0.1, 8, 4.0, 9.0)
    for name, (s, a_s, dq, ds) in cases.items():
        got = N.metrics(p, base_q, s, grey, a_s, 0.1, 0.1, bit, dq, ds)
        assert got == (name == flag), (flag, name)
        assert not N.metrics(p, base_q, s, grey, a_s, 0.1, 0.1, 0, dq, ds)


def _npr_room_case(orc, w=48, h=36):
    from aten_amd.scene import scenedefs
    fs, cam = scenedefs.npr_room()
    c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
    return fs, c, orc.init_sampler(w, h, 0)


def test_two_pass_switch(orc):
    """At 1 spp on npr_room (no stylized shadow) the CPU renderer's literal two-pass OnRender and the one-pass frame agree: frame 0
    byte for byte, later progressive frames within float rounding (contributes_ and the running mean round differently)."""
    w, h = 48, 36
    fs, c, seeds = _npr_room_case(orc, w, h)
    one, two = N.NPR(), N.NPR()
    try:
        for f in range(4):
            a = one.render(fs, c, seeds, w, h, frame=f)
            b = two.render(fs, c, seeds, w, h, frame=f, two_pass=True)
            if f == 0:
                assert np.array_equal(a[..., :3], b[..., :3])
            else:
                np.testing.assert_allclose(a[..., :3], b[..., :3], rtol=1e-5, atol=1e-6)
    finally:
        one.close(); two.close()


def test_lines_sit_on_edges(orc):
    """Oracle-free: every pixel whose sample finds a line at bounce 0 lies within line_width + 1 pixels of a change of the primary
    hit (hit / miss, mesh id, normal, depth or albedo beyond the thresholds the metrics use), and lines are found at all."""
    w, h = 64, 48
    fs, c, seeds = _npr_room_case(orc, w, h)
    o = N.NPR()
    try:
        _, st = o.render(fs, c, seeds, w, h, frame=0, stages=True)
    finally:
        o.close()
    line, pr = st["line"], st["prim"]
    on0 = line["found"] & (line["bounce"] == 0)
    assert on0.sum() > 0.02 * w * h, on0.sum()
    r = int(np.ceil(1.5)) + 1          # npr_room's line width is 1.5 pixels
    bad = []
    for y, x in zip(*np.nonzero(on0)):
        ys, xs = slice(max(0, y - r), y + r + 1), slice(max(0, x - r), x + r + 1)
        hit, mesh = pr["hit"][ys, xs], pr["mesh"][ys, xs]
        nrm, dep, alb = pr["normal"][ys, xs], pr["depth"][ys, xs], pr["albedo_lum"][ys, xs]
        change = (hit != pr["hit"][y, x]).any() or (mesh != pr["mesh"][y, x]).any()
        if not change and pr["hit"][y, x]:
            change = ((1.0 - (nrm * pr["normal"][y, x]).sum(-1)) > 0.1).any() or (np.abs(alb - pr["albedo_lum"][y, x]) > 0.1).any() \
                or (np.abs(dep - pr["depth"][y, x]) > 0.02 * pr["depth"][y, x]).any()
        if not change:
            bad.append((int(x), int(y)))
    assert not bad, bad[:10]


def test_abi_structs():
    """atn_feature_line_config / atn_feature_line_mtrl: sizes, member offsets, and where they sit in the existing structs."""
    src = os.path.join(tempfile.mkdtemp(prefix="npr_abi_"), "abi.cpp")
    with open(src, "w") as f:
        f.write('#include <cstddef>\n#include <cstdio>\n#include "aten_layout.h"\n'
                'int main() { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(atn_feature_line_config), '
                'offsetof(atn_feature_line_config, line_color), offsetof(atn_feature_line_config, line_width), '
                'offsetof(atn_feature_line_config, albedo_threshold), offsetof(atn_feature_line_config, normal_threshold), '
                'sizeof(atn_feature_line_mtrl), offsetof(atn_feature_line_mtrl, metric_flag), '
                'offsetof(atn_scene_rendering_config, feature_line), offsetof(atn_material_param, feature_line)); }\n')
    exe = src[:-4]
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [28, 4, 16, 20, 24, 8, 4, 4, 240]


def test_builder_bytes():
    """SceneBuilder.set_feature_line -> bytes 4-31 of the config; add_material / add_toon_material(feature_line=...) -> bytes
    240-247 of the material; the defaults leave every byte zero (existing uploads unchanged)."""
    import struct
    from aten_amd import layout as L
    from aten_amd.scene.builder import SceneBuilder
    b = SceneBuilder()
    before = bytes(C.string_at(C.addressof(b.config), C.sizeof(b.config)))
    assert before[4:32] == bytes(28)
    b.set_feature_line(True, (0.25, 0.5, 1.0), 2.0, 0.05, 0.2)
    raw = bytes(C.string_at(C.addressof(b.config), C.sizeof(b.config)))
    assert raw[4:32] == struct.pack("<B3x3ffff", 1, 0.25, 0.5, 1.0, 2.0, 0.05, 0.2)
    assert raw[:4] == before[:4] and raw[32:] == before[32:]
    m0 = b.add_material("a", L.MTRL_GGX, (1, 1, 1))
    m1 = b.add_material("b", L.MTRL_GGX, (1, 1, 1), feature_line=(1, 15))
    m2 = b.add_toon_material("c", (1, 1, 1), feature_line=(1, 4))
    rec = lambda i: b.materials[i][1].tobytes()
    assert L.MATERIAL_PARAM.itemsize == 248
    assert rec(m0)[240:248] == bytes(8)
    assert rec(m1)[240:248] == struct.pack("<B3xi", 1, 15)
    assert rec(m2)[240:248] == struct.pack("<B3xi", 1, 4)
    assert rec(m0)[:24] == rec(m1)[:24] and rec(m0)[26:240] == rec(m1)[26:240]      # (24-25: the material id)


def test_library_exports_npr_entry_points():
    from aten_amd import _lib
    for s in ("atn_npr_render", "atn_npr_reset", "atn_npr_capture", "atn_npr_download"):
        assert s in _lib.SYMBOLS
    so = os.environ.get("ATEN_AMD_LIB") or os.path.join(ROOT, "aten_amd", "libaten_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in ("atn_npr_render", "atn_npr_reset", "atn_npr_capture", "atn_npr_download"):
        assert s in names, s
