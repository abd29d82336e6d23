"""The NPR look-through on the CPU (tests/cxx/npr_advance_oracle.cpp, AdvanceNPRPath restated literally): the twin gives npr_oracle's
frame where nothing is looked through, the alpha blend against hand-worked float32 values, the pane in front of the background, the
CheckStencil verdicts by region, the literal re-walk against the last walk (the device's shortcut), the categories the GPU tests
rely on, and the library's new entry points."""
import os
import subprocess

import numpy as np
import pytest

import npr_advance_oracle as A
import npr_advance_scenes as S
import npr_oracle as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    o.lib()
    return o


def _case(orc, scene, w=W, h=H):
    fs, cam = scene
    return fs, orc.create_camera(cam["pos"], cam["at"], cam["vfov"], w, h), orc.init_sampler(w, h, 0)


@pytest.fixture(scope="module")
def rooms(orc):
    """room -> (scene, names, camera, seeds, [(film, stages) of frames 0-3 at 64 x 48, depth 3])"""
    out = {}
    for room, make in S.ROOMS.items():
        scene, names = make()
        fs, c, seeds = _case(orc, scene)
        o = A.NPRAdvance()
        try:
            frames = [o.render(fs, c, seeds, W, H, max_depth=3, frame=f, stages=True) for f in range(4)]
        finally:
            o.close()
        out[room] = (fs, names, c, seeds, frames)
    return out


def _same_stages(a, b):
    for k in ("line", "desc", "disc"):
        for kk in a[k]:
            assert np.array_equal(a[k][kk], b[k][kk]), (k, kk)
    assert np.array_equal(a["terminated"], b["terminated"]) and np.array_equal(a["dims"], b["dims"])


@pytest.mark.parametrize("which,w,h", [("npr_room", 64, 48), ("npr_sponza", 48, 27)])
def test_twin_closure(orc, which, w, h):
    """Nothing to look through means npr_oracle's frame: film and stages byte-equal, and an untouched advance stage."""
    from aten_amd.scene import scenedefs
    fs, c, seeds = _case(orc, getattr(scenedefs, which)(), w, h)
    assert not (fs.arrays["materials"]["stencil_type"] == 2).any() and fs.desc.config.enable_alpha_blending == 0
    a, b = A.NPRAdvance(), N.NPR()
    try:
        for f in range(3):
            fa, sa = a.render(fs, c, seeds, w, h, max_depth=3, frame=f, stages=True)
            fb, sb = b.render(fs, c, seeds, w, h, max_depth=3, frame=f, stages=True)
            assert fa.tobytes() == fb.tobytes(), f
            _same_stages(sa, sb)
            adv = sa["adv"]
            assert not adv["kind"].any() and not adv["walks"].any() and (adv["transmission"] == 1).all() and not adv["throughput"].any()
    finally:
        a.close(); b.close()


def _blend_by_hand(base, alpha, walks):
    """k look-throughs of one pane material: the float32 loop of pathtracing_impl.h:562-566 with a texel of (1, 1, 1, 1)."""
    f = np.float32
    t, thr = f(1.0), np.zeros(3, np.float32)
    one = f(1.0)
    for _ in range(walks):
        thr = thr + ((t * np.asarray(base, np.float32)) * one) * f(alpha)
        t = t * (one - f(alpha))
    return t, thr.astype(np.float32)


def test_blend_hand_worked(rooms):
    """On every pixel that looked through k panes of ONE material with a constant alpha: transmission and throughput, exactly."""
    fs, names, _, _, frames = rooms["alpha"]
    mats = fs.arrays["materials"]
    seen = set()
    for _, st in frames:
        adv = st["adv"]
        for name in ("pane", "skypane", "stack9", "stack11"):
            base = mats["baseColor"][names[name]]
            for k in np.unique(adv["walks"][(adv["mtrl"] == names[name]) & (adv["kind"] == 2)]):
                m = (adv["mtrl"] == names[name]) & (adv["kind"] == 2) & (adv["walks"] == k)
                t, thr = _blend_by_hand(base[:3], base[3], int(k))
                assert (adv["transmission"][m] == t).all(), (name, k)
                assert (adv["throughput"][m] == thr).all(), (name, k)
                assert adv["singular"][m].all()
                seen.add((name, int(k)))
    assert ("stack9", 9) in seen and ("stack11", 10) in seen and ("pane", 1) in seen and ("skypane", 1) in seen, seen


def test_texture_alpha(rooms):
    """The textured pane: texels of alpha 1 are opaque (untouched, and the path stops accumulating), 0.5 and 0 are looked through with
    transmission 0.5 and 1."""
    fs, names, _, _, frames = rooms["alpha"]
    adv = frames[0][1]["adv"]
    m = (adv["mtrl"] == names["texpane"]) & ~frames[0][1]["terminated"]
    ts = set(np.unique(adv["transmission"][m & (adv["kind"] == 2)]).tolist())
    assert ts == {0.5, 1.0}, ts
    assert (m & (adv["kind"] == 0)).sum() >= 10          # the opaque texels
    clear = m & (adv["kind"] == 2) & (adv["transmission"] == 1.0)
    assert clear.any() and not adv["throughput"][clear].any()


def test_pane_in_front_of_background(orc, rooms):
    """max_depth 1: the path that looked through to the background is not shaded and has no depth left -- a black pixel.
    max_depth 2: it misses again at depth 1 and takes ShadeMiss there: transmission * background + throughput (misW 1: is_singular)."""
    fs, names, c, seeds, frames = rooms["alpha"]
    adv = frames[0][1]["adv"]
    m = (adv["mtrl"] == names["skypane"]) & (adv["kind"] == 2) & (adv["answer"] < 0)
    assert m.sum() >= S.FLOOR
    o = A.NPRAdvance()
    try:
        one = o.render(fs, c, seeds, W, H, max_depth=1, frame=0, progressive=False)
        two, st = o.render(fs, c, seeds, W, H, max_depth=2, frame=0, progressive=False, stages=True)
    finally:
        o.close()
    assert not one[m][:, :3].any()
    m2 = m & ~st["line"]["found"]
    assert m2.sum() >= S.FLOOR
    bg = np.array(fs.desc.config.bg.bg_color[:3], np.float32)
    base = fs.arrays["materials"]["baseColor"][names["skypane"]]
    t, thr = _blend_by_hand(base[:3], base[3], 1)
    want = (t * (np.float32(1.0) * bg) + thr) * np.float32(1.0)
    assert (two[m2][:, :3] == want).all(), (two[m2][:3], want)


def test_stencil_verdicts(rooms):
    """CheckStencil by region: what is behind each STENCIL quad decides the verdict, the look-through's answer and the walks."""
    fs, names, _, _, frames = rooms["stencil"]
    tri_mtrl = fs.arrays["triangles"]["mtrlid"]
    expect = {"hair_front": (1, 1), "hair_back": (2, 1), "hair_none": (3, 1), "hair_nothing": (4, 1), "hair_two": (1, 2)}
    for _, st in frames:
        adv = st["adv"]
        live = ~(st["line"]["found"] & (st["line"]["bounce"] == 0))
        for name, (verdict, walks) in expect.items():
            m = (adv["mtrl"] == names[name]) & live
            hit = m & (adv["verdict"] == verdict) & (adv["walks"] == walks)
            assert hit.sum() >= S.FLOOR, (name, hit.sum())
            # (perspective: at a region's rim the ray passes the surface behind and meets the wall -- NONE -- or passes the wall too)
            assert set(np.unique(adv["verdict"][m]).tolist()) <= {verdict, 3, 4}, (name, np.unique(adv["verdict"][m]))
        t = adv["verdict"] == 1
        assert (adv["kind"][t] == 1).all() and (tri_mtrl[adv["answer"][t]] == names["brow"]).all()
        f = (adv["verdict"] >= 2) & live
        # false: the path keeps its hit (blending is off in this room: no alpha check behind it)
        assert (adv["kind"][f] == 0).all() and (tri_mtrl[adv["answer"][f]] == adv["mtrl"][f]).all()
        assert not adv["singular"].any() and (adv["transmission"] == 1).all()


def test_stencil_false_then_alpha(orc):
    """With blending on, a STENCIL surface whose check said false is looked through by its alpha (the check runs on the original hit)."""
    scene, names = S.stencil_room(blending=True)
    fs, c, seeds = _case(orc, scene)
    fs.arrays["materials"]["baseColor"][names["hair_none"]][3] = 0.5
    o = A.NPRAdvance()
    try:
        _, st = o.render(fs, c, seeds, W, H, max_depth=3, frame=0, stages=True)
    finally:
        o.close()
    adv = st["adv"]
    m = (adv["mtrl"] == names["hair_none"]) & (adv["verdict"] == 3)
    assert m.sum() >= S.FLOOR
    assert (adv["kind"][m] == 2).all() and (adv["walks"][m] == 2).all() and (adv["transmission"][m] == 0.5).all()
    assert adv["rewalk_same"].all()


def test_rewalk_is_the_last_walk(rooms):
    """The device takes the last walk's answer where the reference walks the path's ray again: the literal re-walk gives that answer
    on every advanced pixel, the spent budget included."""
    for room in rooms:
        for _, st in rooms[room][4]:
            adv = st["adv"]
            assert (adv["kind"] > 0).sum() > 200
            assert adv["rewalk_same"].all()


@pytest.mark.parametrize("room", sorted(S.ROOMS))
def test_category_floors(rooms, room):
    for f, (_, st) in enumerate(rooms[room][4]):
        counts = S.category_counts(room, st["adv"])
        assert counts and all(v >= S.FLOOR for v in counts.values()), (f, counts)


def test_library_exports_the_entry_points():
    from aten_amd import _lib
    new = ("atn_npr_set_skip_through", "atn_npr_advance_download")
    for s in new:
        assert s in _lib.SYMBOLS
    so = os.environ.get("ATEN_AMD_LIB") or os.path.join(ROOT, "aten_amd", "libaten_amd.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    names = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in new:
        assert s in names, s
    header = open(os.path.join(ROOT, "include", "aten_amd.h")).read()
    for s in new:
        assert "int %s(" % s in header
