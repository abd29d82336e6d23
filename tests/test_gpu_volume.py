"""Volume rendering on the GPU (atn_volume_*, device/volume.hpp) against the CPU restatement of the reference
(tests/cxx/volume_oracle.cpp): the phase table, stage parity after iteration 1, frame parity, Beer-Lambert, the byte-equality rules
and the refused configurations."""
import numpy as np
import pytest

from conftest import make_camera, parity_record, ulp_diff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vq():
    import volume_oracle
    volume_oracle.lib()
    return volume_oracle


def _scene(name):
    from aten_amd.scene import scenedefs
    return getattr(scenedefs, name)()


def _ctx(scene, cam, w, h):
    from aten_amd.renderer import PathTracing
    r = PathTracing(0)
    r.UpdateSceneData(scene)
    r.updateCamera(cam)
    r.initSampler(w, h, 0)
    return r


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-30)


# ---- 8. the phase table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", (-0.9, -0.4, 0.0, 0.4, 0.9))
def test_phase_table(gpu, vq, orc, g):
    fs, cam = _scene("cornell_box")
    r = _ctx(fs, make_camera(orc, cam, 16, 16), 16, 16)
    n = 262144
    rng = np.random.default_rng(int((g + 1) * 100))
    w = rng.normal(size=(n, 3)); w = (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(np.float32)
    wo = rng.normal(size=(n, 3)); wo = (wo / np.linalg.norm(wo, axis=1, keepdims=True)).astype(np.float32)
    r1, r2 = rng.random(n).astype(np.float32), rng.random(n).astype(np.float32)
    got_d, got_e = r.volume_phase_table(g, w, r1, r2, wo)
    want_d, want_e = vq.phase_sample(g, w, r1, r2), vq.phase_eval(g, w, wo)
    ok = np.isfinite(want_d).all(axis=1)          # (the unclamped sqrt: test_volume_oracle_cpu.py)
    assert (~ok).mean() < 1e-3
    err_d = np.abs(got_d[ok] - want_d[ok]).max(axis=1)      # relative to the unit length of a direction
    err_e = _rel(got_e, want_e)
    print("phase table g=%g: direction max %.3g, evaluate max rel %.3g" % (g, err_d.max(), err_e.max()))
    assert err_d.max() <= 2e-5
    assert err_e.max() <= 2e-5


# ---- 9. stage parity after iteration 1 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cornell_box_medium", "cornell_box_smoke"])
def test_stage_parity(gpu, vq, orc, which):
    """Frames 0-3, 96 x 96, the pixels whose primary hit is a Volume material (iteration 0 passed through a boundary).  Their next
    ray after iteration 0 is byte-equal; after iteration 1: stack, stack size, depth_count exact, s within 2 ulp, the event decision
    and the CMJ dimension exact but for pixels whose s and hit distance lie within 4 ulp of each other (at most 1 in 1000), scattered
    directions within 2e-5, the connection's transmittance within 1e-5 relative and its visible flag exact where the connection
    record is bit-equal."""
    fs, cam = _scene(which)
    w = h = 96
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    r = _ctx(fs, c, w, h)
    for f in range(4):
        r.volume_reset()
        r.volume_capture(0)
        r.volume_render(w, h, frame=f)
        g0s, g0r = r.volume_buffer("state"), r.volume_buffer("ray")
        _, w0 = vq.Volume().render(fs, c, seeds, w, h, frame=f, capture=0)
        vol = w0["state"]["passed"] & w0["state"]["processed"]
        assert vol.sum() > 500
        assert np.array_equal(g0s["passed"], w0["state"]["passed"])
        assert np.array_equal(g0r["org"][vol].view(np.uint32), w0["ray"]["org"][vol].view(np.uint32))
        assert np.array_equal(g0r["dir"][vol].view(np.uint32), w0["ray"]["dir"][vol].view(np.uint32))

        r.volume_reset()
        r.volume_capture(1)
        r.volume_render(w, h, frame=f)
        gs, gr, gc, gk = r.volume_buffer("state"), r.volume_buffer("ray"), r.volume_buffer("conn"), r.volume_buffer("stack")
        cnt = r.volume_buffer("counters")
        assert cnt["stack_overflow"] == 0 and cnt["walk_overflow"] == 0
        v = vq.Volume()
        _, ws = v.render(fs, c, seeds, w, h, frame=f, capture=1)
        assert v.counters["stack_overflow"] == 0 and v.counters["walk_overflow"] == 0
        wst, wr, wc = ws["state"], ws["ray"], ws["conn"]
        assert np.array_equal(gs["processed"][vol], wst["processed"][vol]) and wst["processed"][vol].all()
        assert np.array_equal(gs["sampled"][vol], wst["sampled"][vol]) and wst["sampled"][vol].all()
        assert np.array_equal(gr["hit_t"][vol].view(np.uint32), wr["hit_t"][vol].view(np.uint32))
        sd = ulp_diff(gr["s"][vol], wr["s"][vol])
        print("%s frame %d: %d pixels, s max %d ulp" % (which, f, vol.sum(), sd.max()))
        assert sd.max() <= 2
        tie = np.zeros_like(vol)
        tie[vol] = ulp_diff(wr["s"][vol], wr["hit_t"][vol]) <= 4
        assert tie.sum() <= vol.sum() / 1000
        m = vol & ~tie
        for k in ("absorbed", "scattered", "passed", "connection", "terminated"):
            assert np.array_equal(gs[k][m], wst[k][m]), k
        assert np.array_equal(gs["dim"][m], wst["dim"][m])
        assert np.array_equal(gs["depth_count"][m], wst["depth_count"][m])
        assert np.array_equal(gs["stack_size"][m], wst["stack_size"][m])
        assert np.array_equal(gk[m], ws["stack"][m])
        sc = m & wst["scattered"]
        if sc.any():
            dd = np.abs(gr["dir"][sc] - wr["dir"][sc]).max()
            print("   scattered %d, direction max %.3g" % (sc.sum(), dd))
            assert dd <= 2e-5
        same = m & wst["connection"] & np.all(gc["org"].view(np.uint32) == wc["org"].view(np.uint32), -1) \
            & np.all(gc["dir"].view(np.uint32) == wc["dir"].view(np.uint32), -1) & (gc["t_max"].view(np.uint32) == wc["t_max"].view(np.uint32))
        print("   connections %d, bit-equal records %d" % ((m & wst["connection"]).sum(), same.sum()))
        assert same.sum() > 0
        assert np.array_equal(gc["visible"][same], wc["visible"][same])
        assert np.array_equal(gc["segments"][same], wc["segments"][same])
        tr = _rel(gc["transmittance"][same], wc["transmittance"][same])
        assert tr.max() <= 1e-5


# ---- 10. frame parity ---------------------------------------------------------------------------------------------------------------
FLOORS = {"cornell_box": 99.9, "cornell_box_medium": 99.5, "cornell_box_smoke": 99.5, "cornell_box_subsurface": 99.5}


@pytest.mark.parametrize("brk", [True, False])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("which", ["cornell_box_medium", "cornell_box_smoke", "cornell_box_subsurface", "cornell_box"])
def test_frame_parity(gpu, vq, orc, which, spp, brk):
    fs, cam = _scene(which)
    w, h = 256, 144
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    r = _ctx(fs, c, w, h)
    v = vq.Volume()
    worst = 100.0
    for f in range(5):
        got = r.volume_render(w, h, spp=spp, frame=f, break_on_terminate=brk)
        want = v.render(fs, c, seeds, w, h, spp=spp, frame=f, break_on_terminate=brk)
        m = parity_record("volume_%s_spp%d_brk%d_frame%d" % (which, spp, int(brk), f), got, want)
        cnt = r.volume_buffer("counters")
        assert cnt["stack_overflow"] == 0 and cnt["walk_overflow"] == 0
        assert v.counters["stack_overflow"] == 0 and v.counters["walk_overflow"] == 0
        inside = 100.0 * float(np.mean(np.all(np.abs(got - want) <= 1e-3 * np.maximum(1.0, np.abs(want)), axis=-1)))
        mean_rel = abs(float(got[..., :3].mean()) - float(want[..., :3].mean())) / max(float(want[..., :3].mean()), 1e-30)
        print("volume %s spp %d brk %d frame %d: %.3f %% inside, image-mean rel %.3g" % (which, spp, int(brk), f, inside, mean_rel), m)
        worst = min(worst, inside)
        assert mean_rel <= 5e-3
    assert worst >= FLOORS[which]


# ---- 11. Beer-Lambert -----------------------------------------------------------------------------------------------------------------
def test_beer_lambert(gpu, orc):
    from test_volume_oracle_cpu import beer_lambert_check
    state = {}

    def render(scene, cam, w, h, frame, spp):
        if "r" not in state:
            state["r"] = _ctx(scene, make_camera(orc, cam, w, h), w, h)
        return state["r"].volume_render(w, h, spp=spp, frame=frame, break_on_terminate=False)
    dev, se, _ = beer_lambert_check(orc, render)
    print("Beer-Lambert on the GPU: mean deviation %.3g, standard error %.3g" % (dev, se))
    cnt = state["r"].volume_buffer("counters")
    assert cnt["stack_overflow"] == 0 and cnt["walk_overflow"] == 0


# ---- 12. byte-equality ----------------------------------------------------------------------------------------------------------------
def test_byte_equality(gpu, orc):
    fs, cam = _scene("cornell_box_smoke")
    w, h = 128, 96
    c = make_camera(orc, cam, w, h)

    def frames(r, n=4, **kw):
        return [r.volume_render(w, h, spp=2, frame=f, **kw).copy() for f in range(n)]
    a = frames(_ctx(fs, c, w, h))
    b = frames(_ctx(fs, c, w, h))
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # 1 against 4 frames in flight
    r4 = _ctx(fs, c, w, h)
    r4.set_frames_in_flight(4)
    for f in range(4):
        r4.volume_render(w, h, spp=2, frame=f, download=False)
    assert np.array_equal(r4.download_film().view(np.uint32), a[3].view(np.uint32))
    # reset, then frame 0 against a fresh context
    r = _ctx(fs, c, w, h)
    frames(r)
    r.volume_reset()
    assert np.array_equal(r.volume_render(w, h, spp=2, frame=0).view(np.uint32), a[0].view(np.uint32))
    # capture on against capture off
    rc = _ctx(fs, c, w, h)
    rc.volume_capture(1)
    for x, y in zip(a, frames(rc)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_atn_render_unchanged_by_volume_frames(gpu, orc):
    fs, cam = _scene("cornell_box")
    w, h = 128, 96
    r = _ctx(fs, make_camera(orc, cam, w, h), w, h)
    before = r.render(w, h, frame=0).copy()
    r.reset()
    for f in range(3):
        r.volume_render(w, h, frame=f)
    r.volume_reset()
    after = r.render(w, h, frame=0)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


# ---- 13. refusals -----------------------------------------------------------------------------------------------------------------------
ERR_UNSUPPORTED = -5


def _refused(r, w, h, word, **kw):
    with pytest.raises(Exception) as e:
        r.volume_render(w, h, **kw)
    assert "(status %d)" % ERR_UNSUPPORTED in str(e.value), str(e.value)
    assert word in str(e.value), str(e.value)


def test_refusals(gpu, orc):
    import ctypes as C
    from aten_amd import layout as L
    from aten_amd.renderer import Destination
    from aten_amd.scene import scenedefs
    from aten_amd.scene.builder import SceneBuilder
    from aten_amd.scene.scenedefs import _box_mesh
    w, h = 32, 32
    fs, cam = _scene("cornell_box_smoke")
    c = make_camera(orc, cam, w, h)

    def medium_scene(edit=None, extra=None):
        b = SceneBuilder()
        m = b.add_medium_material("fog", 0.0, 0.1, 0.4)
        if edit:
            edit(b.materials[m][1])
        if extra:
            extra(b)
        p, tri = _box_mesh((-1, -1, -1), (1, 1, 1))
        b.create_instance(b.add_mesh("box", p, tri, m))
        b.set_background((1, 1, 1))
        return b.build()

    def grid(m):
        m["medium"][3] = np.int32(0).view(np.float32)

    def zero(m):
        m["medium"][1] = 0.0
        m["medium"][2] = 0.0

    def stencil(b):
        b.materials[b.add_material("st", L.MTRL_DIFFUSE, (1, 1, 1))][1]["stencil_type"] = 2
    _refused(_ctx(medium_scene(grid), c, w, h), w, h, "grid_idx")
    _refused(_ctx(medium_scene(zero), c, w, h), w, h, "sigma_a + sigma_s")
    _refused(_ctx(medium_scene(extra=lambda b: b.add_carpaint_material("paint")), c, w, h), w, h, "CarPaint")
    _refused(_ctx(medium_scene(extra=stencil), c, w, h), w, h, "STENCIL")
    alpha = scenedefs.toon_room(alpha_blocker=True)
    _refused(_ctx(alpha[0], make_camera(orc, alpha[1], w, h), w, h), w, h, "alpha")

    r = _ctx(fs, c, w, h)
    r.set_regeneration(True)
    _refused(r, w, h, "regeneration", spp=2)
    r.set_regeneration(False)
    r.set_shade_math(True)
    _refused(r, w, h, "relaxed")
    r.set_shade_math(False)
    r.setScreenShard(0, 2)
    _refused(r, w, h, "world 1")
    r.setScreenShard(0, 1)
    d = Destination(w, h, 5, 3, 1, 0, 1, 1, 1, 0)                                 # count_stats
    assert r._l.atn_volume_render(r._ctx, C.byref(d), None) == ERR_UNSUPPORTED
    assert b"count_stats" in r._l.atn_last_error(r._ctx)
    # the configuration is back to what is accepted: the scene renders
    assert np.isfinite(r.volume_render(w, h)).all()
    # a scene without media renders
    fs0, cam0 = scenedefs.cornell_box()
    film = _ctx(fs0, make_camera(orc, cam0, w, h), w, h).volume_render(w, h)
    assert np.isfinite(film).all() and film[..., :3].max() > 0
