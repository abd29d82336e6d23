"""Grid media on the GPU (atn_volume_set_grids, device/volume_grid.hpp) against the CPU twin (tests/cxx/volume_grid_oracle.cpp):
stage parity after iterations 0, 1 and 3, connection parity, frame parity, the byte-equality rules, the refusals and the cap counters.
docs/VOLUME.md, "Grid media".  The twin's own gates (near ties at most 0.5 % of pixels, zero caps) are tests/test_volume_grid_cpu.py."""
import numpy as np
import pytest

from conftest import make_camera, parity_record, ulp_diff

pytestmark = pytest.mark.gpu

ERR_UNSUPPORTED = -5
SCENES = ("cornell_box_smoke_grid", "smoke_grid_ragged")
SIZES = ((64, 48), (100, 52))
FRAMES = (0, 1, 2)


@pytest.fixture(scope="module")
def vg():
    import volume_grid_oracle
    volume_grid_oracle.lib()
    return volume_grid_oracle


_scenes = {}


def _scene(name):
    from aten_amd.scene import scenedefs
    if name not in _scenes:
        _scenes[name] = getattr(scenedefs, name)()
    return _scenes[name]


def _ctx(scene, cam, w, h, grids="own"):
    from aten_amd.renderer import PathTracing
    r = PathTracing(0)
    r.UpdateSceneData(scene)
    r.updateCamera(cam)
    r.initSampler(w, h, 0)
    if grids is not None:
        r.volume_set_grids(scene.grids if grids == "own" else grids)
    return r


# the twin's captures, computed once per (scene, size, frame, iteration) and shared by the tests below
_twin = {}


def _twin_stage(vg, orc, name, w, h, frame, it):
    key = (name, w, h, frame, it)
    if key not in _twin:
        fs, cam = _scene(name)
        v = vg.Volume()
        _, st = v.render(fs, make_camera(orc, cam, w, h), orc.init_sampler(w, h, 0), w, h, frame=frame, capture=it)
        _twin[key] = (st, v.counters)
    return _twin[key]


def _capture(r, w, h, frame, it):
    r.volume_reset()
    r.volume_capture(it)
    r.volume_render(w, h, frame=frame)
    out = dict(state=r.volume_buffer("state"), ray=r.volume_buffer("ray"), conn=r.volume_buffer("conn"), stack=r.volume_buffer("stack"))
    out["counters"] = r.volume_buffer("counters")
    out["grid_counters"] = r.volume_buffer("grid_counters")
    return out


# A ray that enters an iteration off the twin's by an ulp-level difference (the libraries' sinf / cosf / powf behind a scatter or a
# BSDF sample: directions lie up to ~1e-6 apart, positions that times the path length) cannot be held to "2 ulp per step of sample_s":
# the clip subtracts coordinates of order 1.  NEAR bounds what counts as the same ray on both sides: 1e-4 absolute in origin and
# direction (the scenes are of order 1), relative in hit_t -- two orders above what the libraries produce, an order above the twin's
# tie band.  Pixels further apart took another branch at an earlier iteration (a near tie there); the frame contract lets 0.5 % of
# the pixels do that, so at most 0.5 % per iteration run so far may.
NEAR = 1e-4
DIVERGED_PER_ITERATION = 0.005


def _check_the_rest(name, w, h, f, it, rest, near, ws, wr, gs, gr):
    """The unmarked pixels that entered the iteration NEAR the twin's ray but not bit-equal to it.  The floor: near pixels are at
    least 1 - 0.5 % x (iterations run) of the processed ones.  The weaker bound: a decision compares numbers moved by up to ~NEAR
    relative, ten times the twin's tie band, so an unmarked pixel may flip, with a probability of the order of NEAR per comparison
    and a handful of comparisons per flight: at least 99 % of these pixels make every decision of the twin's (flags, step count,
    dim, depth_count, stack size), and where they do, sample_s lies within 4 NEAR of the twin's, relative to max(1, |s|) (the two
    ends of the clip and one sum per step), again on 99 % of them: a clip that enters the box at a grazing angle divides the ray's
    difference by a small direction component."""
    processed = ws["processed"].sum()
    assert near.sum() >= (1.0 - DIVERGED_PER_ITERATION * (it + 1)) * processed, (f, it, int(near.sum()), int(processed))
    n = int(rest.sum())
    if n == 0:
        print("%s %dx%d frame %d iteration %d: %d of %d near, none of them off the twin's ray" % (name, w, h, f, it, near.sum(), processed))
        return
    agree = np.ones_like(rest)
    for k in ("sampled", "scattered", "absorbed", "passed", "connection", "terminated", "flight_steps", "dim", "depth_count", "stack_size"):
        agree &= gs[k] == ws[k]
    a = rest & agree
    serr = np.abs(gr["s"][a] - wr["s"][a]) / np.maximum(1.0, np.abs(wr["s"][a])) if a.any() else np.zeros(1)
    print("%s %dx%d frame %d iteration %d: %d of %d near; %d off the twin's ray by an ulp-level difference, %d of them make every decision "
          "of the twin's, s within %.3g (%d of them within %.3g)" % (name, w, h, f, it, near.sum(), processed, n, a.sum(), serr.max(), (serr <= 4 * NEAR).sum(), 4 * NEAR))
    assert a.sum() >= 0.99 * n - 1
    assert (serr <= 4 * NEAR).sum() >= 0.99 * len(serr) - 1


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_stage_and_connection_parity(gpu, vg, orc, name, size):
    """After iterations 0, 1 and 3 of sample 0, frames 0-2.  Pixels that enter the iteration with a ray bit-equal to the twin's (at
    iteration 0 all of them: the primary ray and hit_t are the renderer's own bit-exact values; later the next ray captured after the
    iteration before, since the 2 ulp per step of sample_s are counted from the same ray) and that the twin has not marked as a
    near tie (the rest: _check_the_rest, with a floor on how many there may be): the event flag, the flight's step count, the stack, depth_count and the sampler's dimension are equal; sample_s lies
    within 2 ulp per step; scattered directions within 2e-5.  Connections whose record is bit-equal: segments, visibility, the
    ratio-tracking step count and the final dimension of the connection's stream are equal, the transmittance within 1e-5."""
    w, h = size
    fs, cam = _scene(name)
    r = _ctx(fs, make_camera(orc, cam, w, h), w, h)
    try:
        for f in FRAMES:
            for it in (0, 1, 3):
                want, wcnt = _twin_stage(vg, orc, name, w, h, f, it)
                got = _capture(r, w, h, f, it)
                assert got["grid_counters"] == dict(flight_capped=0, connection_capped=0)
                assert wcnt["flight_capped"] == 0 and wcnt["connection_capped"] == 0
                ws, wr, wc, gs, gr, gc = want["state"], want["ray"], want["conn"], got["state"], got["ray"], got["conn"]
                # the pixels compared: processed on both sides, the ray that entered the iteration bit-equal to the twin's (the next ray
                # the iteration before left behind, and the hit distance found along it), no near tie
                entered = ws["processed"] & gs["processed"] & (gr["hit_t"].view(np.uint32) == wr["hit_t"].view(np.uint32))
                near = ws["processed"] & gs["processed"] & (np.abs(gr["hit_t"] - wr["hit_t"]) <= NEAR * np.maximum(1.0, np.abs(wr["hit_t"])))
                if it > 0:
                    pw, pg = _twin_stage(vg, orc, name, w, h, f, it - 1)[0]["ray"], _capture(r, w, h, f, it - 1)["ray"]
                    for k in ("org", "dir"):
                        entered &= np.all(pg[k].view(np.uint32) == pw[k].view(np.uint32), axis=-1)
                        near &= np.abs(pg[k] - pw[k]).max(axis=-1) <= NEAR
                unmarked = (want["ties"] & 1) == 0
                m = entered & unmarked
                _check_the_rest(name, w, h, f, it, near & ~entered & unmarked, near, ws, wr, gs, gr)
                assert np.array_equal(gs["processed"], ws["processed"]) or it > 0
                rate = entered.sum() / max(1, ws["processed"].sum())
                if it == 0:
                    assert rate == 1.0
                for k in ("sampled", "scattered", "absorbed", "passed", "connection", "terminated"):
                    assert np.array_equal(gs[k][m], ws[k][m]), (k, f, it)
                assert np.array_equal(gs["flight_steps"][m], ws["flight_steps"][m])
                assert np.array_equal(gs["dim"][m], ws["dim"][m])
                assert np.array_equal(gs["depth_count"][m], ws["depth_count"][m])
                assert np.array_equal(gs["stack_size"][m], ws["stack_size"][m])
                assert np.array_equal(got["stack"][m], want["stack"][m])
                sm = m & ws["sampled"]
                sd = ulp_diff(gr["s"][sm], wr["s"][sm]) if sm.any() else np.zeros(1, np.int64)
                assert (sd <= 2 * np.maximum(1, ws["flight_steps"][sm])).all() if sm.any() else True
                sc = m & ws["scattered"]
                derr = np.abs(gr["dir"][sc] - wr["dir"][sc]).max() if sc.any() else 0.0
                assert derr <= 2e-5
                # connections
                cm = m & ws["connection"] & gs["connection"]
                same = cm & np.all(gc["org"].view(np.uint32) == wc["org"].view(np.uint32), axis=-1) \
                    & np.all(gc["dir"].view(np.uint32) == wc["dir"].view(np.uint32), axis=-1) \
                    & (gc["t_max"].view(np.uint32) == wc["t_max"].view(np.uint32)) & ((want["ties"] & 2) == 0)
                assert np.array_equal(gc["segments"][same], wc["segments"][same])
                assert np.array_equal(gc["visible"][same], wc["visible"][same])
                assert np.array_equal(gc["track_steps"][same], wc["track_steps"][same])
                assert np.array_equal(gc["stream_dim"][same], wc["stream_dim"][same])
                terr = np.abs(gc["transmittance"][same] - wc["transmittance"][same]) / np.maximum(np.abs(wc["transmittance"][same]), 1e-30)
                terr = np.where(wc["transmittance"][same] == gc["transmittance"][same], 0.0, terr)
                assert (terr <= 1e-5).all()
                bit_s = float((gr["s"][sm].view(np.uint32) == wr["s"][sm].view(np.uint32)).mean()) if sm.any() else 1.0
                print("%s %dx%d frame %d iteration %d: %d of %d pixels entered bit-equal, %d compared, %d flights (s bit-equal %.4f, max %d ulp), "
                      "%d scatters (dir %.3g), %d of %d connections bit-equal (%d tracked steps)"
                      % (name, w, h, f, it, entered.sum(), ws["processed"].sum(), m.sum(), sm.sum(), bit_s, sd.max(), sc.sum(), derr,
                         same.sum(), cm.sum(), wc["track_steps"][same].sum()))
                if f == 0:
                    parity_record("volume_grid_stage_%s_%dx%d_it%d" % (name, w, h, it), gr["org"], wr["org"], entered_bit_equal=float(rate),
                                  s_bit_equal=bit_s, s_max_ulp=int(sd.max()), connections_bit_equal=int(same.sum()), connections=int(cm.sum()))
                assert m.sum() > 100 and (it == 0 or sm.sum() > 50)
    finally:
        r.close()


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("brk", (True, False))
@pytest.mark.parametrize("spp", (1, 2))
@pytest.mark.parametrize("name", SCENES)
def test_frame_parity(gpu, vg, orc, name, spp, brk, size):
    """3 progressive frames, 64 x 48 and the ragged 100 x 52: at least 99.5 % of the pixels inside 1e-3 * max(1, |twin|), the renderer's contract; both cap
    counters zero."""
    w, h = size
    fs, cam = _scene(name)
    c = make_camera(orc, cam, w, h)
    seeds = orc.init_sampler(w, h, 0)
    r = _ctx(fs, c, w, h)
    v = vg.Volume()
    try:
        for f in FRAMES:
            got = r.volume_render(w, h, spp=spp, frame=f, break_on_terminate=brk)
            want = v.render(fs, c, seeds, w, h, spp=spp, frame=f, break_on_terminate=brk)
            assert r.volume_buffer("grid_counters") == dict(flight_capped=0, connection_capped=0)
            assert v.counters["flight_capped"] == 0 and v.counters["connection_capped"] == 0
            m = parity_record("volume_grid_frame_%s_%dx%d_spp%d_brk%d_f%d" % (name, w, h, spp, int(brk), f), got, want)
            print("%s %dx%d spp %d break %d frame %d: %.4f inside, mean rel err %.3g" % (name, w, h, spp, brk, f, m["frac_within_0.001"], m["image_mean_relerr"]))
            assert m["frac_within_0.001"] >= 0.995
    finally:
        r.close()


@pytest.mark.parametrize("size", SIZES)
def test_the_film_does_not_depend_on_the_walk(gpu, orc, monkeypatch, size):
    """The film of a grid scene (64 x 48 and the ragged 100 x 52) is byte-equal under ATEN_AMD_TRACE=r / s and ATEN_AMD_LDS_NODES=0 / 1: a connection draws from its
    own stream, so which lane walks which connection, and in which order, does not reach the film."""
    w, h = size
    fs, cam = _scene("smoke_grid_ragged")
    c = make_camera(orc, cam, w, h)
    films = {}
    for key, env in (("own", {}), ("refill", dict(ATEN_AMD_TRACE="r")), ("simple", dict(ATEN_AMD_TRACE="s")),
                     ("global", dict(ATEN_AMD_LDS_NODES="0")), ("lds", dict(ATEN_AMD_LDS_NODES="1"))):
        for k in ("ATEN_AMD_TRACE", "ATEN_AMD_LDS_NODES"):
            monkeypatch.delenv(k, raising=False)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        r = _ctx(fs, c, w, h)
        try:
            films[key] = [r.volume_render(w, h, spp=2, frame=f).copy() for f in FRAMES]
        finally:
            r.close()
    assert all(np.isfinite(f).all() for f in films["own"]) and films["own"][-1][..., :3].max() > 0
    for key in films:
        for a, b in zip(films["own"], films[key]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), key


def test_unnamed_grids_change_nothing_and_dropped_grids_are_refused(gpu, orc):
    """Grids that no material names leave cornell_box_smoke byte-equal to a context without grids; volume_set_grids([]) after a grid
    frame brings the grid_idx refusal back, and setting the grids again the frame."""
    w, h = 64, 48
    fs, cam = _scene("cornell_box_smoke")
    gfs, gcam = _scene("cornell_box_smoke_grid")
    c = make_camera(orc, cam, w, h)
    a, b = _ctx(fs, c, w, h, grids=None), _ctx(fs, c, w, h, grids=gfs.grids)
    try:
        for f in FRAMES:
            fa, fb = a.volume_render(w, h, frame=f), b.volume_render(w, h, frame=f)
            assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    finally:
        a.close(); b.close()
    r = _ctx(gfs, make_camera(orc, gcam, w, h), w, h)
    try:
        first = r.volume_render(w, h, frame=0).copy()
        r.volume_set_grids([])
        with pytest.raises(Exception) as e:
            r.volume_render(w, h, frame=1)
        assert "(status %d)" % ERR_UNSUPPORTED in str(e.value) and "grid_idx" in str(e.value), str(e.value)
        r.volume_set_grids(gfs.grids)
        r.volume_reset()
        again = r.volume_render(w, h, frame=0)
        assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    finally:
        r.close()


def _slab(grid_data, **medium):
    """constant_grid_slab's geometry with one medium over grid_data = (density, origin, voxel_size)."""
    from aten_amd.scene import scenedefs
    from aten_amd.scene.builder import SceneBuilder
    b = SceneBuilder()
    kw = dict(g=0.0, sigma_a=0.0, sigma_s=1.0, le=(0.0, 0.0, 0.0), grid=0, majorant=None)
    kw.update(medium)
    b.grids.append(grid_data)
    if kw["majorant"] is None:
        kw["majorant"] = 1.0
    m = b.add_medium_material("slab", kw["g"], kw["sigma_a"], kw["sigma_s"], kw["le"], grid=kw["grid"], majorant=kw["majorant"])
    p, tri = scenedefs._box_mesh((-50.0, -50.0, -1.0), (50.0, 50.0, 0.0))
    b.create_instance(b.add_mesh("slab", p, tri, m))
    b.set_background((1.0, 1.0, 1.0))
    return b.build(), dict(pos=(0.0, 0.0, 2.0), at=(0.0, 0.0, 0.0), vfov=45.0)


def test_refusals(gpu, orc):
    """Every refusal of a grid or of a medium that names one: ATN_ERR_UNSUPPORTED with its message, and the context renders a valid
    frame afterwards."""
    w, h = 32, 24
    ones = np.ones((4, 4, 4), np.float32)
    good = (ones, (-50.0, -50.0, -75.0), 25.0)
    bad_density = ones.copy(); bad_density[1, 2, 3] = np.inf
    neg_density = ones.copy(); neg_density[0, 0, 0] = -0.5
    cases = [
        (good, dict(grid=1), "grid_idx"),
        (good, dict(sigma_a=0.25), "sigma_a == 0"),
        (good, dict(majorant=float("nan")), "majorant"),
        (good, dict(majorant=0.0), "majorant"),
        (good, dict(majorant=0.5), "below sigma_s * max density"),
        (good, dict(sigma_s=8.0, majorant=8.0), "> 1024"),
        ((ones, (0.0, 0.0, 0.0), float("inf")), {}, "voxel_size"),
        ((ones, (0.0, 0.0, 0.0), 0.0), {}, "voxel_size"),
        ((bad_density, good[1], good[2]), {}, "not finite"),
        ((neg_density, good[1], good[2]), {}, "density < 0"),
    ]
    valid = _slab(good)[0]
    for grid_data, medium, word in cases:
        fs, cam = _slab(grid_data, **medium)
        r = _ctx(fs, make_camera(orc, cam, w, h), w, h)
        try:
            with pytest.raises(Exception) as e:
                r.volume_render(w, h)
            assert "(status %d)" % ERR_UNSUPPORTED in str(e.value) and word in str(e.value), (word, str(e.value))
            r.UpdateSceneData(valid)        # (drops the grids)
            r.volume_set_grids([good])
            film = r.volume_render(w, h)
            assert np.isfinite(film).all() and film[..., :3].max() > 0
        finally:
            r.close()
    # n = 0, and a dim component <= 0 (which no array can carry: the struct by hand)
    import ctypes as C
    from aten_amd.renderer import VolumeGrid
    fs, cam = _slab(good)
    r = _ctx(fs, make_camera(orc, cam, w, h), w, h, grids=None)
    try:
        with pytest.raises(Exception) as e:
            r.volume_render(w, h)
        assert "grid_idx" in str(e.value), str(e.value)
        g = VolumeGrid()
        g.dim[:] = [4, 0, 4]
        g.voxel_size = 25.0
        g.density = ones.ctypes.data
        r._check(r._l.atn_volume_set_grids(r._ctx, C.byref(g), 1))
        with pytest.raises(Exception) as e:
            r.volume_render(w, h)
        assert "(status %d)" % ERR_UNSUPPORTED in str(e.value) and "dim component <= 0" in str(e.value), str(e.value)
        r.volume_set_grids([good])
        film = r.volume_render(w, h)
        assert np.isfinite(film).all() and film[..., :3].max() > 0
        assert r.volume_buffer("grid_counters") == dict(flight_capped=0, connection_capped=0)
    finally:
        r.close()
