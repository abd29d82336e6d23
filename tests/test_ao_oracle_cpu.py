"""Ambient occlusion on the CPU: the twin (tests/cxx/ao_oracle.cpp) against hand-worked scenes, the reference's quirks it keeps,
the row rule of the CPU renderer and idaten's miss rule, the bilateral filter, the test scene's skip-throughs and the library's new
entry points."""
import os
import subprocess

import numpy as np
import pytest

import ao_oracle as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = np.float32(3.14159265358979323846)
AO_SYMBOLS = ("atn_ao_set_params", "atn_ao_render", "atn_ao_reset", "atn_ao_capture", "atn_ao_download")


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.lib()
    return o


def test_library_exports_ao_entry_points():
    """The four-plus-one atn_ao_* symbols: in the header, in the binding's list and in the built library's export table."""
    from aten_amd import _lib
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    for s in AO_SYMBOLS:
        assert "int %s(atn_ctx* ctx" % s in header, s
        assert s in _lib.SYMBOLS, s
    so = os.environ.get("ATEN_AMD_LIB") or os.path.join(ROOT, "aten_amd", "libaten_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in AO_SYMBOLS:
        assert s in names, s


def _quad(b, name, y, mtrl, up=True, half=50.0):
    """A horizontal square at height y whose geometric normal points up (or down)."""
    q = np.array([[-half, y, -half], [half, y, -half], [half, y, half], [-half, y, half]], np.float32)
    idx = [[0, 2, 1], [0, 3, 2]] if up else [[0, 1, 2], [0, 2, 3]]
    b.create_instance(b.add_mesh(name, q, idx, mtrl))


def _slabs(ceiling=None, panes=(), cam_y=0.2):
    """A floor at y = 0 under an optional opaque ceiling (normal up, so that c = dot(normal, dir) > 0) and half-transparent panes."""
    from aten_amd import layout as L
    from aten_amd.scene.builder import SceneBuilder
    b = SceneBuilder()
    grey = b.add_material("grey", L.MTRL_DIFFUSE, (0.7, 0.7, 0.7))
    _quad(b, "floor", 0.0, grey)
    if ceiling is not None:
        _quad(b, "ceiling", ceiling, grey)
    if panes:
        glass = b.add_material("pane", L.MTRL_DIFFUSE, (0.9, 0.9, 0.9, 0.5))
        for k, y in enumerate(panes):
            _quad(b, "pane%d" % k, y, glass)
    b.set_background((0.0, 0.0, 0.0))
    # from between the floor and whatever hangs above it, looking down at the floor
    return b.build(), dict(pos=(0.0, cam_y, 3.0), at=(0.0, 0.0, 0.0), vfov=45.0)


def _render(orc, scene, w=48, h=36, **kw):
    fs, cam = scene
    c = orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h)
    seeds = orc.init_sampler(w, h, 0)
    o = A.AO()
    try:
        return o.render(fs, c, seeds, w, h, stages=True, **kw)
    finally:
        o.close()


def _term(t, c, r):
    """One hit's addend, ao_isect.t / ao_radius * c / Diffuse::pdf, over a floor whose normal is +y: pdf = |c| / pi (0 where c == 0:
    the entries of rays that did not hit)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        v = t / r * c / (np.abs(c) / PI)
    return np.where(c != 0, v, np.float32(0)).astype(np.float32)


def _floor_pixels(st):
    """Pixels whose primary hit is the floor: the first AO ray starts at y ~ 0 (ray::Offset lifts it by at most 2^-16 ...)."""
    return (st["state"] == 1) & (np.abs(st["ray"]["org"][..., 1]) < 1e-3)


def test_floor_under_a_ceiling(orc):
    """h = 0.5 < radius = 1: a pixel whose AO ray hits the ceiling has the value t / r * c / (c / pi) in the reference's operation
    order, recomputed in float32 from the captured ray's answer; t and c follow from the captured ray's geometry."""
    r = np.float32(1.0)
    film, st = _render(orc, _slabs(ceiling=0.5), radius=float(r), break_on_terminate=False)
    floor = _floor_pixels(st)
    a = st["answer"]
    hit = floor & (a["kind"] == 1)
    assert hit.sum() > 100 and (floor & (a["kind"] == 0)).sum() > 10
    t, c = a["t"][hit], a["c"][hit]
    want = _term(t, c, r)
    assert want.dtype == np.float32
    assert np.array_equal(st["value"][hit], want)
    d, o = st["ray"]["dir"][hit], st["ray"]["org"][hit]
    np.testing.assert_allclose(c, d[:, 1], atol=2e-7)
    np.testing.assert_allclose(t, (0.5 - o[:, 1]) / d[:, 1], rtol=1e-5)
    # a ray that leaves the radius before it reaches the ceiling's box misses: exactly 1
    assert np.all(st["value"][floor & (a["kind"] == 0)] == 1.0)
    assert np.array_equal(film[..., 0][st["state"] != 0], st["value"][st["state"] != 0])


def test_open_floor_is_one(orc):
    """Nothing above the floor: every AO ray misses and sets the value to 1 -- exactly 1.0 with one ray; with four rays the last
    miss leaves 1 and the division by num_rays makes it 0.25 (kept as written)."""
    film, st = _render(orc, _slabs(), break_on_terminate=False)
    assert (st["state"] == 1).sum() > 100
    assert np.all(st["value"][st["state"] != 0] == 1.0)
    assert np.all(film[st["state"] != 0] == 1.0)
    film, st = _render(orc, _slabs(), num_rays=4, break_on_terminate=False)
    assert np.all(st["value"][st["state"] == 1] == 0.25)
    assert np.all(st["value"][st["state"] == 2] == 1.0)


def test_a_miss_sets_the_value(orc):
    """num_rays = 4: `ao = 1.0` on a miss discards what earlier rays added.  A pixel whose last ray misses is exactly 0.25; one whose
    first ray misses and whose later rays hit is (1 + sum of the later rays) / 4.  The fold is recomputed here in index order."""
    r = np.float32(1.0)
    film, st = _render(orc, _slabs(ceiling=0.5), num_rays=4, radius=float(r), break_on_terminate=False)
    floor = _floor_pixels(st)
    al = st["answers"]
    kind, t, c = al["kind"], al["t"], al["c"]
    ao = np.zeros(kind.shape[:2], np.float32)
    for i in range(4):
        add = _term(t[..., i], c[..., i], r)
        ao = np.where(kind[..., i] == 0, np.float32(1.0), np.where((kind[..., i] == 1) & (c[..., i] > 0), ao + add, ao)).astype(np.float32)
    ao = (ao / np.float32(4)).astype(np.float32)
    assert np.array_equal(st["value"][floor], ao[floor])
    last_misses = floor & (kind[..., 3] == 0)
    assert last_misses.sum() > 20
    assert np.all(st["value"][last_misses] == 0.25)
    first_only = floor & (kind[..., 0] == 0) & np.all(kind[..., 1:] == 1, -1)
    assert first_only.sum() > 5
    # (1 + a) + b + c in float32, as the running sum makes it
    run = np.ones(kind.shape[:2], np.float32)
    for i in (1, 2, 3):
        run = (run + _term(t[..., i], c[..., i], r)).astype(np.float32)
    assert np.array_equal(st["value"][first_only], (run / np.float32(4))[first_only])
    assert np.all(st["value"][first_only] > 0.25)
    # a sum that forgot the reset would differ: some pixel has hits in front of a miss
    hits_then_miss = floor & (kind[..., 0] == 1) & (kind[..., 3] == 0)
    assert hits_then_miss.any()


def test_a_hit_beyond_the_radius(orc):
    """The walk's t_max caps box tests only: a triangle that straddles the radius is returned with t / radius > 1."""
    from aten_amd.scene import scenedefs
    film, st = _render(orc, scenedefs.sponza_lod(), w=64, h=48, radius=1.0)
    a = st["answer"]
    beyond = (st["state"] == 1) & (a["kind"] == 1) & (a["t"] > 1.0)
    assert beyond.sum() >= 5


def test_ten_skip_throughs_add_nothing(orc):
    """Twelve panes over the floor: every AO ray that climbs spends its ten walks on panes and adds nothing.  Nine panes under an
    opaque ceiling: nine skip-throughs, then the hit counts."""
    panes = [0.1 + 0.02 * k for k in range(12)]      # the camera sits under the lowest one
    film, st = _render(orc, _slabs(panes=panes, cam_y=0.05), break_on_terminate=False)
    floor = _floor_pixels(st)
    a = st["answer"]
    spent = floor & (a["kind"] == 2)
    assert spent.sum() > 50
    assert np.all(a["skips"][spent] == 10)
    assert np.all(st["value"][spent] == 0.0)
    film, st = _render(orc, _slabs(ceiling=0.4, panes=panes[:9], cam_y=0.05), break_on_terminate=False)
    floor = _floor_pixels(st)
    a = st["answer"]
    through = floor & (a["kind"] == 1) & (a["skips"] == 9)
    assert through.sum() > 50
    assert np.all(st["value"][through] > 0.0)


def test_row_rule(orc):
    """atrium(detail=0.25) at 64 x 48, the CPU renderer as written: in every row the unwritten pixels are exactly {x >= first miss}.
    idaten's switch writes every pixel and differs only on that set."""
    from aten_amd.scene import scenedefs
    scene = scenedefs.atrium(detail=0.25)
    w, h = 64, 48
    lit, sl = _render(orc, scene, w=w, h=h, break_on_terminate=True)
    ida, si = _render(orc, scene, w=w, h=h, break_on_terminate=False)
    first = sl["first_miss"]
    assert sorted(first[first < w].tolist()) == sorted([37, 19, 19, 19, 19, 20, 20])
    assert (si["state"] == 2).sum() == 153
    assert np.array_equal(first, si["first_miss"])
    xs = np.arange(w)[None, :]
    unwritten = xs >= first[:, None]
    assert np.array_equal(lit[..., 3] == 0, unwritten)
    assert np.all(lit[unwritten] == 0)
    assert np.array_equal(sl["state"] == 0, xs > first[:, None])
    assert np.array_equal(sl["state"] == 2, xs == first[:, None])
    assert np.all(ida[..., 3] == 1)
    assert np.array_equal(ida[~unwritten], lit[~unwritten])
    assert np.all(ida[si["state"] == 2][:, :3] == 1.0)


def test_cornell_box_writes_nothing(orc):
    """The Cornell box at 4:3 has a primary miss at x = 0 of every row: the CPU renderer as written puts no pixel."""
    from aten_amd.scene import scenedefs
    film, st = _render(orc, scenedefs.cornell_box(), w=64, h=48)
    assert np.all(st["first_miss"] == 0)
    assert not film.any()
    ida, si = _render(orc, scenedefs.cornell_box(), w=64, h=48, break_on_terminate=False)
    assert (si["state"] == 2).sum() == 288
    assert np.all(ida[..., 3] == 1)


def test_ao_room_skips_through_its_pane(orc):
    """scenedefs.ao_room(): at least 50 AO rays skip through the pane at 64 x 48 with the default radius."""
    from aten_amd.scene import scenedefs
    film, st = _render(orc, scenedefs.ao_room(), w=64, h=48, radius=1.0, break_on_terminate=False)
    assert int((st["answer"]["skips"] > 0).sum()) >= 50
    assert int(st["skips"].sum()) >= 50


def test_filter():
    """ApplyBilateralFilter x 2 and the halving: a constant plane passes through both passes (1 stays 1, 0.5 becomes 0.5 * 0.5 / 2); a
    depth step keeps the two sides apart, the same values over one depth bleed."""
    h, w = 12, 16
    depth = np.full((h, w), 2.0, np.float32)
    assert np.all(A.bilateral(np.ones((h, w), np.float32), depth) == 1.0)
    assert np.all(A.bilateral(np.full((h, w), 0.5, np.float32), depth) == 0.125)
    v = np.ones((h, w), np.float32); v[:, w // 2:] = 0.5
    step = depth.copy(); step[:, w // 2:] = 50.0
    out = A.bilateral(v, step)
    assert np.all(out[:, :w // 2] == 1.0)
    np.testing.assert_allclose(out[:, w // 2:], 0.125, atol=1e-6)
    bleed = A.bilateral(v, depth)
    assert np.all(bleed[:, w // 2 - 1] < 0.5) and np.all(bleed[:, 0] == 1.0)
    # a miss has depth inf: its weights are NaN, the pass falls back to 1
    inf = depth.copy(); inf[:, :3] = np.inf
    assert np.all(A.bilateral(v, inf)[:, :3] == 1.0)


def test_filter_frame(orc):
    """RenderAOWithBilateralFilter on a frame is the filter over the frame's own planes."""
    from aten_amd.scene import scenedefs
    scene = scenedefs.ao_room()
    plain, sp = _render(orc, scene, w=64, h=48, num_rays=3, break_on_terminate=False, progressive=False)
    filt, sf = _render(orc, scene, w=64, h=48, num_rays=3, break_on_terminate=False, progressive=False, filter=True)
    assert np.array_equal(sp["value"], sf["value"])
    assert np.array_equal(filt[..., 0], A.bilateral(sp["value"], sp["depth"]))
    assert np.all(filt[..., 3] == 1)
